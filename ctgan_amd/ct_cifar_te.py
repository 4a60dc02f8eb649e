"""Temporal-ensembling CT classifier for CIFAR-10: TH/CT_CIFAR-10_TE.py (TH/ = CT-GANs/Theano_classifier of the reference), the
variant of TH/CT_CIFAR.py whose consistency term is taken against TEMPORALLY ENSEMBLED TARGETS instead of a second dropout pass.
`CifarTETrainer` for the two steps and the tables, `train()` for the script's loop; the network, the generator, the generator step,
the augmenting gather, the data class, Theano-form Adam with averages, the rotated coordinates and the Philox streams are those of
ct_cifar.py (read its docstring first) and are imported from it, not copied.

What the script shares with TH/CT_CIFAR.py: the classifier (:65-88) and generator (:62-71), the generator step (:148-157, L1 feature
matching on a noisy pass over [G(z) ; x_unl2]), the labelled pick (:160-169), the per-epoch permutations (:194-205) - `rng` is drawn in
the same order, so ct_cifar.CifarSSLData serves as it is -, the reflect padding, flips and windows (:51, :221-271), Adam and the
parameter averages (:138-141), the test pass (:130-131, :144).  What differs:

Settings (:21-23, :119, :215).  factor_M = 0 (Config.FACTOR_M), LAMBDA_2 = 1, prediction_decay = 0.6 (PREDICTION_DECAY); the feature
term has weight 0.1 (FEAT_WEIGHT) INSIDE the hinge; the data-dependent init runs on the first 1000 padded rows (INIT_ROWS), not 500.

Classifier step (:102-126, :143).  Three noisy passes - labelled, unlabelled ONCE, G(z) - run as one stacked 3B-row batch
[lab ; unl ; fake] (TH/CT_CIFAR.py stacks 4B rows).  With t_i [10] and t2_i [128] the target rows of unlabelled example i:
    ct_i  = mean_k (softmax(u_i)_k - softmax(t_i)_k)^2      (the targets are raw ensembled logits, softmaxed here)
    ctf_i = mean_j (f_ij - t2_ij)^2                         (f: the pooled features, disc_layers[-2])
    CT_i  = LAMBDA_2 (ct_i + FEAT_WEIGHT ctf_i) - FACTOR_M,   CT_ = mean_i max(CT_i, 0)
    loss_unl = (CT_ - mean lse(u) + mean softplus(lse(u)) + mean softplus(lse(fake))) / 2
loss_lab, train_err and train_err2 as in TH/CT_CIFAR.py; cost = loss_lab + UNLABELED_WEIGHT loss_unl; the targets are constants.
Beside the scalars the step returns the unlabelled logits and features OF THIS SAME NOISY PASS (:143), which the loop files under
the examples' indices (:300-302).  All of this is functional.te_head - one forward launch that reads the target rows by index and
stores the prediction rows by index, one backward launch (csrc/ssl_te.hip).

Tables and loop (:177-180, :203-207, :273-276, :289-309).  Six per-example tables over the N training examples:
    ensemble [N,10], ensemble2 [N,128]         the running sums  ens = 0.6 ens + 0.4 epoch_pred   (epoch end)
    targets [N,10], targets2 [N,128]           ens / (1 - 0.6^(epoch+1)), taken at the epoch's end: constant within an epoch
    epoch_pred [N,10], epoch_pred2 [N,128]     this epoch's predictions, zero at every epoch's start
`indices_all`, the epoch's first full permutation (CifarSSLData.i_unl), orders the classifier's unlabelled rows AND names their
table rows; the generator's unlabelled batch comes from the second, independent permutation (i_unl2) and touches no table.  The
script keeps the tables in numpy, copies every step's predictions to the host and scatters them in a Python loop; here the tables
live on the device, the head gathers and scatters inside the (graph-replayed) step, and `end_epoch()` is two elementwise launches
(kernels.te_ensemble_update).
Table contract: the tables are allocated by `bind_data` (zeroed) and from then on changed IN PLACE only (the captured graphs hold
their addresses); the unlabelled indices of one batch are distinct - they are slices of a permutation -, duplicates stay
memory-safe but leave an unspecified one of the rows; an index outside [0, N) makes loss_unl NaN and touches no row.

Kept quirks.  In epoch 0 the targets are zeros: softmax(t) is uniform and the feature target is 0 - there is no ramp-up.  A row no
batch of the epoch visited (a shortened epoch, or N no multiple of B) contributes a ZERO prediction to its ensemble.  The report
line's `gen loss` is the SUM over the epoch (:299, never divided); the line starts with `Epoch %d`.  The third augmented copy
(:249-271) and `scipy.linalg` (:16) feed nothing: there is NO ZCA whitening in the script, and none here.

Random numbers.  ct_cifar's streams; the step counter advances by one per generator init pass, classifier init pass, classifier
step and generator step.  Stream ids (rank 0):
    generator init   0  z [B, Z_DIM]
    classifier init  0  input dropout over [INIT_ROWS, 3, 36, 36]     1, 2  dropout after layers 3 and 6
    classifier step  0  z     1  input dropout over the stacked [3B, 3, 32, 32]     2, 3  dropout after layers 3 and 6
                     16 augmentation of the labelled rows             17  augmentation of the unlabelled rows
    generator step   0  z     1  input dropout over the stacked [2B, 3, 32, 32]     2, 3  dropout after layers 3 and 6
                     16 augmentation of the unlabelled rows
Pass p of the stacked classifier batch owns samples [pB, (p+1)B): 0 labelled, 1 unlabelled, 2 generated.

Configuration.  ct_cifar's network functions read `ct_cifar.cfg`; this module's Config extends ct_cifar.Config and `configure()` (and
the construction of a trainer) installs it there, so that both modules see one object.  ct_cifar.configure() puts that module's own
back.
"""
import torch

from . import ct_cifar as C
from . import ct_common
from . import functional as F
from . import kernels as K
from . import tflib as lib
from .ct_cifar import SID_AUG_LAB, SID_AUG_UNL, CifarSSLData, CifarSSLTrainer, Classifier, Generator  # noqa: F401


class Config(C.Config):
    """The literals of TH/CT_CIFAR-10_TE.py:21-30, :62-88, :119, :215 where they differ from ct_cifar.Config, and the two it adds."""
    INIT_ROWS = 1000
    LAMBDA_2 = 1.0
    FACTOR_M = 0.0
    FEAT_WEIGHT = 0.1
    PREDICTION_DECAY = 0.6


cfg = Config()


def configure(**kw):
    """A fresh Config for this module, installed as ct_cifar.cfg too (the imported network, gather and data class read that)."""
    global cfg
    cfg = Config(**kw)
    C.cfg = cfg
    return cfg


class CifarTETrainer(CifarSSLTrainer):
    """train_batch_disc / train_batch_gen (:143, :157), init_param (:142), test_batch (:144) and the six tables of the loop.  Batches
    in the internal form of ct_cifar.CifarSSLTrainer; `i_unl` (int32, device) names the table rows of the unlabelled batch: a
    classifier batch is (x_lab, labels, x_unl, i_unl), train_iteration (:289-299) takes it followed by x_unl2."""
    D_KEYS = ('out8', 'loss_lab', 'loss_unl', 'loss_ct', 'train_err', 'train_err2', 'ct', 'ctf')
    REPORT = ('Epoch',) + CifarSSLTrainer.REPORT[1:]

    def __init__(self, seed=None, data=None):
        C.cfg = cfg
        self.epoch = 0
        self.ensemble = self.ensemble2 = self.targets = self.targets2 = self.epoch_pred = self.epoch_pred2 = None
        super().__init__(seed=seed, data=data)

    def d_cotangents(self):
        """out8 = {loss_lab, loss_unl, CT_, train_err, train_err2, mean ct, mean ctf, 0}: cost = loss_lab + UNLABELED_WEIGHT loss_unl (:138)"""
        return {'out8': [1.0, cfg.UNLABELED_WEIGHT, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]}

    # ---- the device-resident set and the tables over it (:177-180, :273-274)
    def bind_data(self, images_u8):
        """The uint8 training set [N, 3, IMG, IMG] the index batches refer to; allocates the six tables for its N rows, zeroed, and
        puts the epoch count at 0."""
        super().bind_data(images_u8)
        n, nc, fd = self.data.shape[0], cfg.N_CLASSES, cfg.D_WIDTHS[-1]
        z = lambda w: torch.zeros(n, w, dtype=torch.float32, device=self.dev)          # noqa: E731
        self.ensemble, self.targets, self.epoch_pred = z(nc), z(nc), z(nc)
        self.ensemble2, self.targets2, self.epoch_pred2 = z(fd), z(fd), z(fd)
        self.epoch = 0

    def tables(self):
        return {'ensemble': self.ensemble, 'ensemble2': self.ensemble2, 'targets': self.targets, 'targets2': self.targets2,
                'epoch_pred': self.epoch_pred, 'epoch_pred2': self.epoch_pred2}

    # ---- classifier step
    def d_losses(self, x_lab, labels, x_unl, i_unl):
        assert self.targets is not None, 'bind the uint8 training set first (bind_data allocates the tables)'
        B = x_lab.shape[0]
        self.rng.begin_step()
        with torch.no_grad():
            fake = C._generator(B, rng=self.rng)
        logits, feat = C._classifier(C._stack([x_lab, x_unl, fake]), rng=self.rng, features='both')
        out8 = F.te_head(logits, feat, labels, i_unl, self.targets, self.targets2, self.epoch_pred, self.epoch_pred2, B, cfg.LAMBDA_2,
                         cfg.FEAT_WEIGHT, cfg.FACTOR_M)
        return {'out8': out8, 'loss_lab': out8[0], 'loss_unl': out8[1], 'loss_ct': out8[2], 'train_err': out8[3], 'train_err2': out8[4],
                'ct': out8[5], 'ctf': out8[6], 'logits': logits, 'features': feat}

    # ---- the same from index batches: i_unl feeds the gather and names the table rows
    def d_body_idx(self, i_lab, labels, i_unl):
        return self.d_body(self.gather(i_lab, SID_AUG_LAB), labels, self.gather(i_unl, SID_AUG_UNL), i_unl)

    # ---- epoch end (:305-309; :273-274 for the next epoch)
    def end_epoch(self):
        """ens = decay ens + (1 - decay) epoch_pred, targets = ens / (1 - decay^(epoch+1)), epoch_pred = 0 for both table triples (one
        launch each); advances the epoch count."""
        K.te_ensemble_update(self.ensemble, self.targets, self.epoch_pred, cfg.PREDICTION_DECAY, self.epoch)
        K.te_ensemble_update(self.ensemble2, self.targets2, self.epoch_pred2, cfg.PREDICTION_DECAY, self.epoch)
        self.epoch += 1

    # ---- what a checkpoint carries beside checkpoint.save's own (its `extra`)
    def te_state(self):
        """The ensembles, the targets and the epoch count, on the host.  Taken at an epoch boundary (after end_epoch), where the two
        prediction tables are zero; they are not carried."""
        return {'te_epoch': int(self.epoch), 'ensemble': self.ensemble.cpu(), 'ensemble2': self.ensemble2.cpu(), 'targets': self.targets.cpu(),
                'targets2': self.targets2.cpu()}

    def load_te_state(self, state):
        """Restores te_state() into the bound tables in place (the prediction tables are zeroed)."""
        for k in ('ensemble', 'ensemble2', 'targets', 'targets2'):
            t = getattr(self, k)
            if t is None or tuple(t.shape) != tuple(state[k].shape):
                raise ValueError('table %s: the checkpoint has %s, the bound set needs %s' % (k, tuple(state[k].shape), None if t is None else tuple(t.shape)))
            t.copy_(state[k])
        self.epoch_pred.zero_()
        self.epoch_pred2.zero_()
        self.epoch = int(state['te_epoch'])

    checkpoint_extra = te_state

    def restore_extra(self, path, epoch):
        from . import checkpoint
        self.load_te_state(checkpoint.load_extra(path))
        assert self.epoch == epoch, 'the checkpoint was not written at an epoch boundary'


def train(data_dir=None, epochs=None, seed=None, seed_data=None, use_graphs=True, out_dir=None, resume=None, checkpoint_every=1, log=print,
          max_batches=None, arrays=None):
    """The loop of TH/CT_CIFAR-10_TE.py:187-337 on the CIFAR-10 python batches under `data_dir` (or `arrays`, see ct_cifar.CifarSSLData):
    the data-dependent init on the first 1000 padded rows of the first epoch's labelled stream, then per epoch one classifier and one
    generator step per batch (graph replay unless use_graphs=False; gathers, target reads and prediction writes are part of the
    classifier graph - nothing of the tables is copied to the host within an epoch), `end_epoch()`, the test error on the averaged
    parameters and the script's `Epoch %d, ...` line (also one record of train_log.Series in `out_dir`/log.jsonl).  A checkpoint
    (checkpoint.py, the tables in its `extra`) is written to `out_dir` every `checkpoint_every` epochs; `resume` continues from one
    at the epoch it was written.  max_batches: shorten the epochs (smoke runs; unvisited rows then decay, as in the script).
    Returns the trainer."""
    from .engine import GraphedCifarTETrainer
    C.cfg = cfg
    data = CifarSSLData(data_dir, seed=seed, seed_data=seed_data, arrays=arrays)
    lib.delete_all_params()
    return ct_common.train_loop(CifarTETrainer(seed=seed, data=data.train_x), data, GraphedCifarTETrainer, C.init_from_stream, epochs, use_graphs,
                                out_dir, resume, checkpoint_every, log, max_batches)
