"""Semi-supervised CT classifier for CIFAR-10: TH/CT_CIFAR.py with the parts of TH/nn.py it uses (TH/ = CT-GANs/Theano_classifier of
the reference).  `Classifier(inputs)` / `Generator(n_samples)` in the shape of the other script modules, `CifarSSLTrainer` for the two
steps, `CifarSSLData` for the labelled pick, the per-epoch index streams and the device-resident uint8 set, `train()` for the script's loop.

Classifier D (TH/CT_CIFAR.py:79-93), every conv / NIN / dense layer weight-normalised (TH/nn.py:49-104: W = W_param g / sqrt(1e-6 + sum
of W_param^2 per output channel), the layer's bias replaced by a per-channel b added after the conv): dropout 0.2 -> 3x3 conv 128
twice -> 3x3 conv 128 stride 2 -> dropout 0.5 -> 3x3 conv 256 twice -> 3x3 conv 256 stride 2 -> dropout 0.5 -> 3x3 conv 512 WITHOUT
padding (8x8 -> 6x6) -> NIN 256 -> NIN 128, all with LeakyReLU 0.2 -> global mean pool (the FEATURES, disc_layers[-2]) -> dense to the
10 logits (no nonlinearity, train_g, init_stdv 0.1).  Trainable: every W and b, and g of the LAST layer only; the other g are set once
by the data-dependent init and never trained.  Generator G (:69-77): z ~ U[0,1) [B,50] -> Dense 8192 (N(0,0.05), no bias) + batch norm
(batch statistics, eps 1e-6 inside the root, offset, no gain) + ReLU -> [B,512,4,4] -> 5x5 stride-2 transposed conv 256 + BN + ReLU
-> the same to 128 -> weight-normalised 5x5 stride-2 transposed conv to 3 channels, tanh (train_g, init_stdv 0.1; the norm runs per
OUTPUT channel).  The batch norm's running averages are never read by the script and are not kept; its gain-free form runs on bn.hip
with a constant ones gain.

Classifier step (:105-147): four noisy passes - labelled, unlabelled twice (two dropout draws on the same images), G(z) - run as ONE
stacked 4B-row batch [lab ; unl ; unl ; fake]; cost = loss_lab + UNLABELED_WEIGHT loss_unl with
loss_unl = 0.05 mean (feat(unl) - feat(unl2))^2 + (mean (softmax(unl) - softmax(unl2))^2 - mean lse(unl) + mean softplus(lse(unl)) +
mean softplus(lse(fake))) / 2 - functional.ssl_head with lam2 = 1, M = 0 plus functional.feature_consistency, which also carries
train_err2 = mean(max_k logits_lab <= 0).  Only D moves; every trained parameter's average moves by avg += 1e-4 (p - avg) from ZERO.
Generator step (:152-160): loss_gen = mean_j |mean_i feat(x_unl)_ij - mean_i feat(G(z))_ij| over a noisy pass on [G(z) ; x_unl] with
D's parameters as constants; only G moves.  Theano-form Adam (optim.FlatAdamTheano), beta1 0.5, lr 0.0003 constant.  Init (:101-103,
:205): one generator pass with init=True on a fresh z, then one classifier pass with init=True and DROPOUT ON over the first 500 rows
of the epoch's labelled stream - which at that point are still the reflect-padded 36x36 images (kept: the stack runs
36-36-36-18-18-18-9-7 in this one pass).  Test error: the deterministic pass over the unpadded 32x32 test images on the averaged
parameters, with the live g of layers 1-9.  The report line's `gen loss` is the SUM over the epoch's batches (:288, never divided), kept.

Rotated coordinates.  Theano's `pad=1` stride-2 conv on an even size reads pads (1, 0) and its `border_mode='half'` stride-2 transposed
conv is the data gradient of a conv with pads (2, 1); this project's TF-SAME kernels have (0, 1) and (1, 2) - the mirror image.  With R
the rotation of the two spatial axes by 180 degrees:  conv_theano(x; W) = R conv_same(R x; R W)  and  deconv_theano(z; W) =
R deconv_same(R z; R W);  stride-1 SAME, 1x1 and unpadded layers are symmetric (the unpadded conv is the centre of the SAME result,
functional.crop) and the global pool removes R.  So D_theano(x; W) = D_same(R x; R W) and G_theano(z; W) = R G_same(z; R W, dense columns
permuted): the whole network runs on the SAME kernels on rotated maps, the two R between G and D cancel inside the steps, real images
are rotated for free inside the gather (kernels.aug_gather, rot180) and only `Generator()`, `Classifier()` and `predict()` - which
take and return images in the reference's orientation - rotate at their boundary.  The registry holds the ROTATED filters in this
project's layouts; against the script's parameters (conv W [out,in,k,k], Deconv W [in,out,k,k], dense W [in,out]):
    Classifier.i.W [k,k,in,out]  (i = 1..7)   W[r,s,c,o] = W_th[o,c,k-1-r,k-1-s]      Classifier.8/9/10.W [in,out] = W_th (NIN and dense)
    Generator.2/3/4.W [k,k,out,in]            W[r,s,o,i] = W_th[i,o,k-1-r,k-1-s]
    Generator.1.W [Z_DIM, C S S]              column (c, h, w) = column (c, S-1-h, S-1-w) of W_th;  Generator.1.bn_b permuted alike
and every g, b, bn_b per channel unchanged.  tests/ssl_cifar_oracle.py (`load_into_registry`) implements exactly this.

Data (:38-62, :162-265).  x = (-127.5 + uint8) / 255 through a 256-entry table built with the loader's own expression; the uint8 set
stays on the device and kernels.aug_gather reads a batch's rows by index: reflect padding by 2 through index arithmetic, a horizontal
flip with p = 0.5 and a 32x32 window at an offset in 0..4 per axis - the script's 150,000-iteration host loop per epoch (whose draws come
from the global, unseeded np.random: no parity exists to keep) - here drawn per batch from the Philox streams below.  400 labelled
examples per class after a `seed_data` permutation; per epoch 13 permutations of the 4000 labelled rows and two independent
permutations of all 50000 (`unl`, `unl2`), drawn in the script's order.  The script's third augmented copy feeds nothing and is not made.

Random numbers.  Device Philox4x32-10 streams (csrc/philox.h, rng.DeviceRNG) addressed by (seed, stream id, step, element), which
oracle/philox.py regenerates (`uniform`).  The step counter advances by one per generator init pass, classifier init pass, classifier
step and generator step.  Stream ids (rank 0):
    generator init   0  z [B, Z_DIM]
    classifier init  0  input dropout over [INIT_ROWS, 3, 36, 36]     1, 2  dropout after layers 3 and 6
    classifier step  0  z     1  input dropout over the stacked [4B, 3, 32, 32]     2, 3  dropout after layers 3 and 6
                     16 augmentation of the labelled rows             17  augmentation of the unlabelled rows
    generator step   0  z     1  input dropout over the stacked [2B, 3, 32, 32]     2, 3  dropout after layers 3 and 6
                     16 augmentation of the unlabelled rows (the gathers run before the step they feed, at its counter value)
z: element (r, c) is value r Z_DIM + c.  Augmentation: row r takes values 3r (flip if > 0.5), 3r + 1 and 3r + 2 (row / column offset
min(int(5 u), 4)).  Dropout: an element is kept where floor(keep + u) = 1 and scaled by 1 / keep; the kernels draw by the PHYSICAL
index of the channels-last, rotated tensor: logical position (n, c, h, w) of a site over [N, C, H, W] - in the reference's orientation -
takes value ((n H + (H-1-h)) W + (W-1-w)) C + c.  Pass p of a stacked batch owns samples [pB, (p+1)B).
"""
import os

import numpy as np
import torch

from . import ct_common
from . import functional as F
from . import kernels as K
from . import tflib as lib
from .tflib.ops import wn_conv as _wn

SID_AUG_LAB, SID_AUG_UNL = 16, 17      # stream ids of the augmenting gathers (outside the call-site numbering of a step)


class Config(ct_common.Config):
    """The literals of TH/CT_CIFAR.py:17-27, :69-93, :123, :142-144 (tests shrink IMG, the widths and the batch sizes)."""
    SEED = 2
    SEED_DATA = 2
    COUNT = 400
    BATCH_SIZE = 100
    UNLABELED_WEIGHT = 1.
    LR = 0.0003
    BETA1 = 0.5
    BETA2 = 0.999
    AVG_RATE = 0.0001
    EPOCHS = 1000
    INIT_ROWS = 500
    Z_DIM = 50
    PAD = 2
    DROP_IN = 0.2
    DROP_HIDDEN = 0.5
    FEAT_WEIGHT = 0.05
    G_INIT_STDV = 0.1
    D_INIT_STDV = 0.1
    N_CLASSES = 10
    CHANNELS = 3
    IMG = 32
    D_WIDTHS = (128, 128, 128, 256, 256, 256, 512, 256, 128)
    G_WIDTHS = (512, 256, 128)


cfg = Config()


def configure(**kw):
    global cfg
    cfg = Config(**kw)
    return cfg


def byte_table():
    """float32 [256]: the loader's expression (cifar10_data.py `unpickle`: float64 arithmetic, then the cast) on every byte value."""
    return np.asarray((-127.5 + np.arange(256, dtype=np.uint8)) / np.float32(255.0), dtype=np.float32)


_ONES = {}


def _ones(c, dev):
    key = (int(c), str(dev))
    if key not in _ONES:
        _ONES[key] = torch.ones(1, c, dtype=torch.float32, device=dev)
    return _ONES[key]


def _bn_relu(name, x):
    """nn.batch_norm(..., g=None) + ReLU (TH/nn.py:194-216): bn.hip with a constant ones gain, eps 1e-6."""
    c = x.shape[1]
    offset = lib.param(name + '.bn_b', lambda r: np.zeros((c,), dtype='float32'))
    return F.batch_norm(x, _ones(c, x.device), offset.view(1, c), None, 1, True, 1e-6, f64_stats=True)


def rot180(x):
    """R of the module docstring on a [n, c, h, w] tensor, channels-last (the boundary of the public functions; not on the step's path)."""
    return K.to_channels_last(torch.flip(x, (2, 3)))


def _generator(n_samples, noise=None, rng=None, init=False, frozen=False):
    """G in rotated coordinates -> [n_samples, CHANNELS, IMG, IMG]."""
    if noise is None:
        noise = rng.uniform(n_samples, cfg.Z_DIM)
    s0, w = cfg.IMG // 8, cfg.G_WIDTHS
    W1 = lib.param('Generator.1.W', lambda r: r.normal(0.0, _wn.W_STD, (cfg.Z_DIM, w[0] * s0 * s0)).astype('float32'))
    h = _bn_relu('Generator.1', F.linear(noise, W1)).view(n_samples, w[0], s0, s0)
    for i in (1, 2):
        name = 'Generator.%d' % (i + 1)
        Wi = lib.param(name + '.W', lambda r, i=i: r.normal(0.0, _wn.W_STD, (5, 5, w[i], w[i - 1])).astype('float32'))
        h = _bn_relu(name, F.conv2d_transpose(h, Wi, None, stride=2))
    return _wn.WNDeconv2D('Generator.4', w[2], cfg.CHANNELS, 5, h, nonlinearity='tanh', train_g=True, init_stdv=cfg.G_INIT_STDV, init=init,
                          frozen=frozen)


def _classifier(x, init=False, deterministic=False, rng=None, features=False, frozen=False):
    """D in rotated coordinates on a channels-last [n, CHANNELS, S, S] batch.  features: False -> logits; True -> the pooled features;
    'both' -> (logits, features)."""
    kw = dict(init=init, deterministic=deterministic, rng=rng, frozen=frozen)
    w, keep = cfg.D_WIDTHS, 1.0 - cfg.DROP_HIDDEN
    h = F.dropout(x, 1.0 if deterministic else 1.0 - cfg.DROP_IN, rng=rng)
    h = _wn.WNConv2D('Classifier.1', cfg.CHANNELS, w[0], 3, h, **kw)
    h = _wn.WNConv2D('Classifier.2', w[0], w[1], 3, h, **kw)
    h = _wn.WNConv2D('Classifier.3', w[1], w[2], 3, h, stride=2, drop_keep=keep, **kw)
    h = _wn.WNConv2D('Classifier.4', w[2], w[3], 3, h, **kw)
    h = _wn.WNConv2D('Classifier.5', w[3], w[4], 3, h, **kw)
    h = _wn.WNConv2D('Classifier.6', w[4], w[5], 3, h, stride=2, drop_keep=keep, **kw)
    h = _wn.WNConv2D('Classifier.7', w[5], w[6], 3, h, pad=0, **kw)
    h = _wn.WNNIN('Classifier.8', w[6], w[7], h, **kw)
    h = _wn.WNNIN('Classifier.9', w[7], w[8], h, **kw)
    feat = F.spatial_mean(h)
    if features is True:
        return feat
    logits = _wn.WNLinear('Classifier.10', w[8], cfg.N_CLASSES, feat, nonlinearity=None, train_g=True, init_stdv=cfg.D_INIT_STDV, **kw)
    return (logits, feat) if features == 'both' else logits


def Generator(n_samples, noise=None, rng=None, init=False):
    """:69-77 -> [n_samples, 3, IMG, IMG] in (-1, 1), in the reference's orientation.  `noise`: z given; else one uniform call site."""
    return rot180(_generator(n_samples, noise, rng, init))


def Classifier(inputs, init=False, deterministic=False, rng=None, features=False, frozen=False):
    """:79-93 on images [n, 3, S, S] in the reference's orientation -> logits [n, N_CLASSES]; features=True: the pooled features
    (disc_layers[-2]); 'both': (logits, features)."""
    return _classifier(rot180(inputs), init, deterministic, rng, features, frozen)


def build_params():
    """Register every parameter (lib.param creates on first use) with one tiny deterministic pass."""
    with torch.no_grad():
        _classifier(_generator(2, noise=torch.zeros(2, cfg.Z_DIM, device=lib._dev())), deterministic=True)


def _stack(parts):
    """Row-stack channels-last batches into one channels-last batch."""
    return K.to_channels_last(torch.cat(parts, 0))


class CifarSSLTrainer(ct_common.SSLTrainerBase):
    """The Theano functions train_batch_disc / train_batch_gen (:147, :160), init_param (:146) and test_batch (:148).  The step methods
    take image batches in the INTERNAL form - rotated, channels-last, as `gather` / `gather_fixed` write them (or `rot180` of images in
    the reference's orientation); `predict` and `test_error` take the reference's orientation / the uint8 set.  A classifier batch
    is (x_lab, labels, x_unl), train_iteration (:277-288) takes it followed by x_unl2."""
    cfg = property(lambda self: cfg)
    D_KEYS = ('out4', 'out2', 'loss_lab', 'loss_unl', 'loss_comp', 'loss_feat', 'train_err', 'train_err2')
    REPORT = ('Iteration', (('loss_lab', 'loss_lab'), ('loss_unl', 'loss_unl'), ('train err', 'train_err'), ('train err2', 'train_err2')),
              (('gen loss', 'loss_gen'),))

    def __init__(self, seed=None, data=None):
        super().__init__(build_params, seed)
        self.lut = torch.from_numpy(byte_table()).to(self.dev)
        self.data = None
        if data is not None:
            self.bind_data(data)

    def d_cotangents(self):
        """out4 = {loss_lab, loss_unl head, CT, train_err}, out2 = {feature consistency, train_err2}:
        cost = loss_lab + UNLABELED_WEIGHT (head + FEAT_WEIGHT consistency)   (:123, :142)"""
        return {'out4': [1.0, cfg.UNLABELED_WEIGHT, 0.0, 0.0], 'out2': [cfg.UNLABELED_WEIGHT * cfg.FEAT_WEIGHT, 0.0]}

    # ---- the device-resident uint8 set
    def bind_data(self, images_u8):
        """images_u8: uint8 [N, 3, IMG, IMG] (numpy or tensor) - the training set the index batches refer to."""
        t = torch.as_tensor(images_u8)
        assert t.dtype == torch.uint8 and t.dim() == 4
        self.data = t.to(self.dev).contiguous()

    def gather(self, idx, sid, data=None, out=None):
        """Augmented IMG x IMG windows of rows idx (int32, device) drawn from stream `sid` at the current step counter."""
        return K.aug_gather(self.data if data is None else data, idx, self.lut, cfg.IMG, cfg.PAD, spec=(self.rng.seed, sid, self.rng.ctr), out=out)

    def gather_fixed(self, idx, win=None, offset=None, data=None):
        """Unaugmented windows: the unpadded images by default; win = IMG + 2 PAD, offset (0, 0): the reflect-padded ones."""
        return K.aug_gather(self.data if data is None else data, idx, self.lut, cfg.IMG if win is None else win, cfg.PAD, offset=offset)

    # ---- data-dependent init (:101-103, :205)
    def init_params(self, x):
        """x: the init batch in internal form (the padded images: gather_fixed(idx, IMG + 2 PAD, (0, 0)))."""
        self.rng.begin_step()
        with torch.no_grad():
            _generator(cfg.BATCH_SIZE, rng=self.rng, init=True)
        self.rng.end_step()
        self.rng.begin_step()
        with torch.no_grad():
            _classifier(x, init=True, rng=self.rng)
        self.rng.end_step()
        lib.bump_epoch('Generator')
        lib.bump_epoch('Classifier')

    # ---- classifier step
    def d_losses(self, x_lab, labels, x_unl):
        B = x_lab.shape[0]
        self.rng.begin_step()
        with torch.no_grad():
            fake = _generator(B, rng=self.rng)
        logits, feat = _classifier(_stack([x_lab, x_unl, x_unl, fake]), rng=self.rng, features='both')
        out4, ct_i = F.ssl_head(logits, labels, B, 1.0, 0.0)
        out2 = F.feature_consistency(feat, B, logits)
        with torch.no_grad():
            loss_unl = K.axpby(out4[1:2], out2[0:1], 1.0, cfg.FEAT_WEIGHT)[0]
        return {'out4': out4, 'out2': out2, 'loss_lab': out4[0], 'loss_unl': loss_unl, 'loss_comp': out4[2], 'loss_feat': out2[0],
                'train_err': out4[3], 'train_err2': out2[1], 'logits': logits, 'features': feat}

    # ---- generator step
    def g_losses(self, x_unl):
        B = x_unl.shape[0]
        self.rng.begin_step()
        fake = _generator(B, rng=self.rng)
        feats = _classifier(_stack([fake, x_unl]), rng=self.rng, features=True, frozen=True)
        return {'loss_gen': F.feature_matching_l1(feats, B)}

    # ---- the same from index batches into the bound uint8 set: the gathers run at the counter value of the step they feed
    def d_body_idx(self, i_lab, labels, i_unl):
        return self.d_body(self.gather(i_lab, SID_AUG_LAB), labels, self.gather(i_unl, SID_AUG_UNL))

    def g_body_idx(self, i_unl2):
        return self.g_body(self.gather(i_unl2, SID_AUG_LAB))

    def train_iteration_idx(self, i_lab, labels, i_unl, i_unl2):
        self.d_opt.set_lr(self.lr())
        out = self.d_body_idx(i_lab, labels, i_unl)
        self.g_opt.set_lr(self.lr())
        out.update(self.g_body_idx(i_unl2))
        self.iteration += 1
        return out

    # ---- evaluation on the averaged parameters (:132-133, :145, :148)
    def predict(self, x, averaged=True):
        """Logits of the deterministic pass over images in the reference's orientation; averaged: every trained classifier parameter
        replaced by its average (`givens`, :145) - the g of layers 1-9 are not trained, have no average and stay live."""
        return self._averaged(lambda: _classifier(rot180(x), deterministic=True), averaged)

    def test_error(self, images_u8, y, averaged=True, batch_size=None):
        """Mean over whole batches of the per-batch argmax error (:295-298) over a uint8 set [N, 3, IMG, IMG] (unpadded, unaugmented)."""
        bs = batch_size or cfg.BATCH_SIZE
        data = torch.as_tensor(images_u8).to(self.dev).contiguous()
        y = np.asarray(y)
        errs = []
        for t in range(len(y) // bs):
            idx = torch.arange(t * bs, (t + 1) * bs, dtype=torch.int32, device=self.dev)
            logits = self._averaged(lambda: _classifier(self.gather_fixed(idx, data=data), deterministic=True), averaged)
            errs.append(float(np.mean(logits.cpu().numpy().argmax(1) != y[t * bs:(t + 1) * bs])))
        return float(np.mean(errs))


class CifarSSLData:
    """Host side of TH/CT_CIFAR.py:38-62, :162-193: the `cifar-10-batches-py` files (tflib/cifar10.py's reader) or `arrays` with
    x_train / x_test uint8 [n, 3, S, S] (or [n, 3 S S]) and y_train / y_test; COUNT labelled examples per class picked after a `seed_data`
    permutation; per epoch the labelled stream (ceil(N / n_labelled) permutations of the labelled rows) and two independent
    permutations of the whole set, in the script's draw order.  Hands out INDEX batches into `train_x`; nothing is downloaded."""

    def __init__(self, data_dir=None, count=None, seed=None, seed_data=None, batch_size=None, arrays=None, n_classes=None):
        from .tflib import cifar10
        count = cfg.COUNT if count is None else count
        self.batch_size = cfg.BATCH_SIZE if batch_size is None else batch_size
        n_classes = cfg.N_CLASSES if n_classes is None else n_classes
        if arrays is None:
            d = data_dir
            if d is not None and os.path.isdir(os.path.join(d, 'cifar-10-batches-py')):
                d = os.path.join(d, 'cifar-10-batches-py')
            if d is None or not os.path.isfile(os.path.join(d, cifar10.TRAIN_FILES[0])):
                raise IOError("Couldn't find the CIFAR-10 python batches under %s (they are not downloaded)" % data_dir)
            tr = [cifar10._read_batch_file(os.path.join(d, n)) for n in cifar10.TRAIN_FILES]
            te = [cifar10._read_batch_file(os.path.join(d, n)) for n in cifar10.TEST_FILES]
            arrays = {'x_train': np.concatenate([p[0] for p in tr]), 'y_train': np.concatenate([p[1] for p in tr]),
                      'x_test': np.concatenate([p[0] for p in te]), 'y_test': np.concatenate([p[1] for p in te])}

        def images(a):
            a = np.asarray(a)
            assert a.dtype == np.uint8
            return np.ascontiguousarray(a.reshape(a.shape[0], cfg.CHANNELS, cfg.IMG, cfg.IMG))

        self.train_x, self.train_y = images(arrays['x_train']), np.asarray(arrays['y_train']).astype(np.int32)
        self.test_x, self.test_y = images(arrays['x_test']), np.asarray(arrays['y_test']).astype(np.int32)
        n = self.train_x.shape[0]
        self.nr_batches_train = n // self.batch_size
        # :33-36 - the script's `rng` seeds Theano's and lasagne's generators with its first two draws, then shuffles the epochs
        self.rng = np.random.RandomState(cfg.SEED if seed is None else seed)
        self.rng.randint(2 ** 15); self.rng.randint(2 ** 15)
        data_rng = np.random.RandomState(cfg.SEED_DATA if seed_data is None else seed_data)
        inds = data_rng.permutation(n)                       # :163-172; the unlabelled copies (:52-53) keep the file order
        ys = self.train_y[inds]
        self.lab_idx = np.concatenate([inds[ys == j][:count] for j in range(n_classes)]).astype(np.int32)
        self.lab_y = self.train_y[self.lab_idx]
        self.i_lab = self.y_lab = self.i_unl = self.i_unl2 = None

    def begin_epoch(self):
        """:184-193, in the script's draw order."""
        n, nl = self.train_x.shape[0], self.lab_idx.shape[0]
        ii, yy = [], []
        for _ in range(int(np.ceil(n / float(nl)))):
            p = self.rng.permutation(nl)
            ii.append(self.lab_idx[p]); yy.append(self.lab_y[p])
        self.i_lab, self.y_lab = np.concatenate(ii), np.concatenate(yy)
        self.i_unl = self.rng.permutation(n).astype(np.int32)
        self.i_unl2 = self.rng.permutation(n).astype(np.int32)
        return self.nr_batches_train

    def init_indices(self):
        """Rows of the init batch: the first INIT_ROWS of the current epoch's labelled stream (:205)."""
        return self.i_lab[:cfg.INIT_ROWS]

    def batch(self, t):
        """(i_lab, labels, i_unl, i_unl2) of batch t of the current epoch (:277-287)."""
        s = slice(t * self.batch_size, (t + 1) * self.batch_size)
        return self.i_lab[s], self.y_lab[s], self.i_unl[s], self.i_unl2[s]

    def test_set(self):
        return self.test_x, self.test_y


def init_from_stream(trainer, data):
    """The data-dependent init on the padded images of data.init_indices() (:205; after the first begin_epoch())."""
    idx = torch.from_numpy(np.ascontiguousarray(data.init_indices())).to(trainer.dev)
    trainer.init_params(trainer.gather_fixed(idx, cfg.IMG + 2 * cfg.PAD, (0, 0)))


def train(data_dir=None, epochs=None, seed=None, seed_data=None, use_graphs=True, out_dir=None, resume=None, checkpoint_every=1, log=print,
          max_batches=None, arrays=None):
    """The loop of TH/CT_CIFAR.py:175-313 on the CIFAR-10 python batches under `data_dir` (or `arrays`, see CifarSSLData): the
    data-dependent init on the first 500 padded rows of the first epoch's labelled stream, then per epoch one classifier and one
    generator step per batch (graph replay unless use_graphs=False; the augmenting gathers are part of the graphs), the test error on
    the averaged parameters, and the script's report line (also one record of train_log.Series in `out_dir`/log.jsonl).  A checkpoint
    (checkpoint.py) is written to `out_dir` every `checkpoint_every` epochs; `resume` continues from one at the epoch it was written.
    max_batches: shorten the epochs (smoke runs).  Returns the trainer."""
    from .engine import GraphedCifarSSLTrainer
    data = CifarSSLData(data_dir, seed=seed, seed_data=seed_data, arrays=arrays)
    lib.delete_all_params()
    return ct_common.train_loop(CifarSSLTrainer(seed=seed, data=data.train_x), data, GraphedCifarSSLTrainer, init_from_stream, epochs, use_graphs,
                                out_dir, resume, checkpoint_every, log, max_batches)
