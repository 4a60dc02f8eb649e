"""64x64 CT-WGAN: `GoodGenerator` / `GoodDiscriminator` of TF/CT_gan_64x64.py:166-221,357-373
(MODE 'wgan-ct', the architecture pair the script selects, :48) on the shared unconditional CT-WGAN step
(dcgan_step.DCGANTrainer): generator with batch norm, critic with Layernorm (:87-92) - so the gradient penalty
differentiates the normalisation twice - Adam(1e-4, beta1 = 0, beta2 = 0.9) without decay (:561-565).

`Config.ARCH` selects one of the other pairs `GeneratorAndDiscriminator()` lists (:41-72, the ARCHS table below) for the script's
'wgan' / 'dcgan' / 'lsgan' branches, which call the critic with one argument and read one output (:490-537)."""
from . import functional as F
from . import kernels as K
from .dcgan_step import CT_MODE, GanMode, validate_mode
from .tflib.ops import batchnorm as _bn
from .tflib.ops import conv2d as _conv2d
from .tflib.ops import deconv2d as _deconv2d
from .tflib.ops import layernorm as _ln
from .tflib.ops import linear as _linear


# MODE -> objective, optimizer literals, clip, critic steps per iteration (:490-579, :634-646).  Every mode but 'wgan-ct' normalises the
# critic with BatchNorm (Normalize).  'wgan-gp' is named in the script's comment (:30) but its branches raise (:540, :579).
MODES = {
    'wgan-ct': CT_MODE,
    'wgan': GanMode('wgan', 'rmsprop', lr=5e-5, clip=0.01),                               # :492-494, :548-558
    'dcgan': GanMode('bce', 'adam', lr=2e-4, betas=(0.5, 0.999), critic_iters=1),        # :521-533, :566-570
    'lsgan': GanMode('ls', 'rmsprop', lr=1e-4, critic_iters=1),                          # :535-537, :572-576
}


# ARCH -> (generator, critic) of GeneratorAndDiscriminator() (:41-72); the functions are defined below.  'resnet101' (:69-70) is listed by the
# script and not built here.
ARCHS = ('good', 'dcgan', 'wganpaper', 'fc', 'dcgan-nobn', 'multiplicative', 'dcgan-tanh')
UNBUILT_ARCHS = ('resnet101',)


def validate_arch(arch, mode):
    if arch in UNBUILT_ARCHS:
        raise NotImplementedError('%s: ARCH %r (the 101-layer bottleneck ResnetGenerator / ResnetDiscriminator, :297, :402) is not built' % (__name__, arch))
    if arch not in ARCHS:
        raise NotImplementedError('%s: ARCH %r is not supported (supported: %s)' % (__name__, arch, ', '.join(sorted(ARCHS))))
    if arch != 'good' and mode == 'wgan-ct':
        raise NotImplementedError("%s: ARCH %r has no MODE 'wgan-ct' - the CT branch calls the critic with (x, dim, kp1, kp2, kp3) and reads a "
                                  "feature output, which only GoodDiscriminator has (:494-500); use MODE 'wgan', 'dcgan' or 'lsgan'" % (__name__, arch))


class Config:
    """UPPERCASE globals of TF/CT_gan_64x64.py:27-37 (+ ARCH: the line of GeneratorAndDiscriminator() left uncommented, :41-72)."""
    LAMBDA_2 = 2.0
    Factor_M = 0.0
    MODE = 'wgan-ct'
    ARCH = 'good'
    DIM = 64
    CRITIC_ITERS = 5
    BATCH_SIZE = 64
    ITERS = 200000
    LAMBDA = 10
    OUTPUT_DIM = 64 * 64 * 3
    LR = 1e-4

    def __init__(self, **kw):
        for k, v in kw.items():
            if not hasattr(Config, k):
                raise AttributeError('unknown hyper-parameter %s' % k)
            setattr(self, k, v)
        validate_mode(__name__, MODES, self.MODE)
        validate_arch(self.ARCH, self.MODE)


cfg = Config()
ADAM_BETAS = (0.0, 0.9)
GEN_TOWERS = 1
PIECEWISE_LINEAR_CRITIC = False


def configure(**kw):
    global cfg
    cfg = Config(**kw)
    return cfg


# real_prep's divisor: with it the trainer's augmentation converts the integer pixels on load (kernels.diffaug, one launch for both)
REAL_DENOM = 255.0


def real_prep(real_data_int):
    """:483  2*((int/255.)-.5)"""
    return K.real_prep(real_data_int, None, REAL_DENOM)


def image_shape():
    """(channels, height, width) of the flat NCHW images (the trainer's augmentation, kernels.diffaug)."""
    return (3, 64, 64)


def feat_shapes():
    """Dropout sites: after Res2 [4*DIM,16,16], Res3 [8*DIM,8,8], Res4 [8*DIM,4,4] (:362-367); the other ARCHs' critics have no dropout."""
    if cfg.ARCH != 'good':
        return []
    D = cfg.DIM
    return [(4 * D, 16, 16), (8 * D, 8, 8), (8 * D, 4, 4)]


def Normalize(name, axes, inputs, relu=False, groups=1):
    """:87-92 (+ build-only `groups`: independent BatchNorm statistic groups of a batched generator forward)"""
    if ('Discriminator' in name) and (cfg.MODE == 'wgan-ct'):
        if axes != [0, 2, 3]:
            raise Exception('Layernorm over non-standard axes is unsupported')
        return _ln.Layernorm(name, [1, 2, 3], inputs, relu=relu)      # ReLU fused into the Layernorm kernels
    return _bn.Batchnorm(name, axes, inputs, fused=True, relu=relu, groups=groups)


def ConvMeanPool(name, input_dim, output_dim, filter_size, inputs, he_init=True, biases=True, resid=None):
    """:107-110 (conv + mean pool = one stride-2 conv with the spread filter when the channel counts allow)"""
    return _conv2d.Conv2D(name, input_dim, output_dim, filter_size, inputs, he_init=he_init, biases=biases, pool=True, resid=resid)


def MeanPoolConv(name, input_dim, output_dim, filter_size, inputs, he_init=True, biases=True):
    """:112-116"""
    return _conv2d.Conv2D(name, input_dim, output_dim, filter_size, F.mean_pool2(inputs), he_init=he_init, biases=biases)


def UpsampleConv(name, input_dim, output_dim, filter_size, inputs, he_init=True, biases=True):
    """:118-125"""
    return _conv2d.Conv2D(name, input_dim, output_dim, filter_size, inputs, he_init=he_init, biases=biases, x_up=True)


def ResidualBlock(name, input_dim, output_dim, filter_size, inputs, resample=None, he_init=True, groups=1):
    """:127-162 (Conv1 has no bias, :157).  `groups`: statistic groups of the BatchNorms (generator; the critic outside MODE 'wgan-ct')."""
    if resample not in (None, 'down', 'up'):
        raise Exception('invalid resample value')
    if output_dim == input_dim and resample is None:
        shortcut = inputs
    elif resample == 'down':
        shortcut = MeanPoolConv(name + '.Shortcut', input_dim, output_dim, 1, inputs, he_init=False, biases=True)
    elif resample == 'up':
        shortcut = UpsampleConv(name + '.Shortcut', input_dim, output_dim, 1, inputs, he_init=False, biases=True)
    else:
        shortcut = _conv2d.Conv2D(name + '.Shortcut', input_dim, output_dim, 1, inputs, he_init=False, biases=True)
    out = Normalize(name + '.BN1', [0, 2, 3], inputs, relu=True, groups=groups)
    if resample == 'up':
        out = UpsampleConv(name + '.Conv1', input_dim, output_dim, filter_size, out, he_init=he_init, biases=False)
        out = Normalize(name + '.BN2', [0, 2, 3], out, relu=True, groups=groups)
        return _conv2d.Conv2D(name + '.Conv2', output_dim, output_dim, filter_size, out, he_init=he_init, resid=shortcut)
    out = _conv2d.Conv2D(name + '.Conv1', input_dim, input_dim, filter_size, out, he_init=he_init, biases=False)
    out = Normalize(name + '.BN2', [0, 2, 3], out, relu=True, groups=groups)
    if resample == 'down':
        return ConvMeanPool(name + '.Conv2', input_dim, output_dim, filter_size, out, he_init=he_init, resid=shortcut)
    return _conv2d.Conv2D(name + '.Conv2', input_dim, output_dim, filter_size, out, he_init=he_init, resid=shortcut)


def Generator(n_samples, noise=None, rng=None, groups=1):
    """GoodGenerator :204-221.  `groups` > 1 (build-only): that many generator calls in one batch, each with its own BatchNorm
    statistics (dcgan_step.DCGANTrainer.generate_fakes).  cfg.ARCH other than 'good': that ARCH's generator (ARCH_NETS)."""
    dim = cfg.DIM
    if noise is None:
        noise = rng.normal(n_samples, 128)
    if cfg.ARCH != 'good':
        return ARCH_NETS[cfg.ARCH][0](noise, groups)
    out = _linear.Linear('Generator.Input', 128, 4 * 4 * 8 * dim, noise)
    out = F.to_channels_last(out.reshape(-1, 8 * dim, 4, 4))
    out = ResidualBlock('Generator.Res1', 8 * dim, 8 * dim, 3, out, resample='up', groups=groups)
    out = ResidualBlock('Generator.Res2', 8 * dim, 4 * dim, 3, out, resample='up', groups=groups)
    out = ResidualBlock('Generator.Res3', 4 * dim, 2 * dim, 3, out, resample='up', groups=groups)
    out = ResidualBlock('Generator.Res4', 2 * dim, 1 * dim, 3, out, resample='up', groups=groups)
    out = Normalize('Generator.OutputN', [0, 2, 3], out, relu=True, groups=groups)
    out = _conv2d.Conv2D('Generator.Output', 1 * dim, 3, 3, out, out_nchw=True)
    out = F.tanh(out)
    return out.reshape(-1, cfg.OUTPUT_DIM)


def critic_is_per_sample():
    """Layernorm (MODE 'wgan-ct') normalises each sample on its own; a batch-normalised critic couples the rows of a batch."""
    return cfg.MODE == 'wgan-ct' and cfg.ARCH == 'good'


def DiscriminatorTrunk(inputs, groups=1):
    """Input conv + Res1 + Res2: everything before the first dropout (:358-363); deterministic and per-sample (MODE 'wgan-ct'), shared by
    the two dropout passes over the real batch of a critic step (dcgan_step.DCGANTrainer.d_losses).  `groups`: the critic calls batched in
    `inputs`, each with its own statistics (BatchNorm critic of the other modes)."""
    dim = cfg.DIM
    out = inputs.reshape(-1, 3, 64, 64)
    out = _conv2d.Conv2D('Discriminator.Input', 3, dim, 3, out, he_init=False)
    out = ResidualBlock('Discriminator.Res1', dim, 2 * dim, 3, out, resample='down', groups=groups)
    return ResidualBlock('Discriminator.Res2', 2 * dim, 4 * dim, 3, out, resample='down', groups=groups)


def DiscriminatorTail(h, kp1=0.8, kp2=0.5, kp3=0.5, u=None, rng=None, groups=1):
    """dropout -> Res3 -> dropout -> Res4 -> dropout -> Linear (:364-373)."""
    dim = cfg.DIM

    def drop(i, x, kp):
        if kp == 1.0:
            return x
        return F.dropout(x, kp, u[i]) if u is not None else F.dropout(x, kp, rng=rng)
    out = drop(0, h, kp1)
    out = ResidualBlock('Discriminator.Res3', 4 * dim, 8 * dim, 3, out, resample='down', groups=groups)
    out = drop(1, out, kp2)
    out = ResidualBlock('Discriminator.Res4', 8 * dim, 8 * dim, 3, out, resample='down', groups=groups)
    out = drop(2, out, kp3)
    output2 = F.to_nchw(out).reshape(-1, 4 * 4 * 8 * dim)
    out = _linear.Linear('Discriminator.Output', 4 * 4 * 8 * dim, 1, output2)
    return out.reshape(-1), output2


def Discriminator(inputs, kp1=0.8, kp2=0.5, kp3=0.5, u=None, rng=None, groups=1):
    """GoodDiscriminator :357-373 -> (D [n], D_ [n, 4*4*8*DIM]).  cfg.ARCH other than 'good': that ARCH's critic (ARCH_NETS) -> (D [n], None);
    it has no dropout (kp*, u and rng are unused)."""
    if cfg.ARCH != 'good':
        return ARCH_NETS[cfg.ARCH][1](inputs, groups), None
    return DiscriminatorTail(DiscriminatorTrunk(inputs, groups), kp1, kp2, kp3, u=u, rng=rng, groups=groups)


def build_params(device=None):
    import torch
    from . import tflib as lib
    if device is not None:
        lib.set_device(device)
    dev = lib._dev()
    with torch.no_grad():
        x = Generator(2, noise=torch.zeros(2, 128, device=dev))
        Discriminator(x, 1.0, 1.0, 1.0)


# ----------------------------------------------------------------------------------------------------------------- the other ARCHs
def _stdev(on):
    """set_weights_stdev(0.02) / unset_weights_stdev() on conv2d, deconv2d and linear (:238-240, :269-271, :438-440, :463-465)."""
    for m in (_conv2d, _deconv2d, _linear):
        m.set_weights_stdev(0.02) if on else m.unset_weights_stdev()


def _hidden(name, x, act, bn, groups):
    """[Batchnorm over [0,2,3]] + nonlinearity of a hidden layer: act 'relu' (folded into bn.hip's launches), 'lrelu' / 'tanh' / 'gate' (folded
    into bn_act.hip's; CTGAN_BN_ACT_FUSED=0: the separate launches).  Without BN the activation's own launch."""
    if bn:
        if act == 'relu':
            return _bn.Batchnorm(name, [0, 2, 3], x, fused=True, relu=True, groups=groups)
        return _bn.Batchnorm(name, [0, 2, 3], x, fused=True, groups=groups, act=act)
    return {'relu': F.relu, 'lrelu': F.leaky_relu, 'tanh': F.tanh, 'gate': F.gate}[act](x)


def _deconv_generator(noise, groups, act, bn, width, stdev):
    """DCGANGenerator :237-273 (act 'relu' / 'tanh', bn, width (8, 4, 2, 1)), MultiplicativeDCGANGenerator :325-353 (act 'gate': twice the
    channels in front of each gate) and WGANPaper_CrippledDCGANGenerator :275-295 (no BN, width (1, 1, 1, 1); its ReLU at :280 sits in front
    of the reshape - elementwise, so the same values)."""
    dim = cfg.DIM
    m = 2 if act == 'gate' else 1
    w = [k * dim for k in width]
    if stdev:
        _stdev(True)
    try:
        out = _linear.Linear('Generator.Input', 128, 4 * 4 * w[0] * m, noise)
        out = F.to_channels_last(out.reshape(-1, w[0] * m, 4, 4))
        out = _hidden('Generator.BN1', out, act, bn, groups)
        for i in (2, 3, 4):
            out = _deconv2d.Deconv2D('Generator.%d' % i, w[i - 2], w[i - 1] * m, 5, out)
            out = _hidden('Generator.BN%d' % i, out, act, bn, groups)
        out = _deconv2d.Deconv2D('Generator.5', w[3], 3, 5, out)
    finally:
        if stdev:
            _stdev(False)
    return F.tanh(F.to_nchw(out)).reshape(-1, cfg.OUTPUT_DIM)


def FCGenerator(noise, groups=1, FC_DIM=512):
    """:223-235 - four ReLULayers (Linear(initialization='he'), :79-81) and the output Linear; the rows are independent (no BN)."""
    out, n_in = noise, 128
    for i in (1, 2, 3, 4):
        out = F.relu(_linear.Linear('Generator.%d.Linear' % i, n_in, FC_DIM, out, initialization='he'))
        n_in = FC_DIM
    return F.tanh(_linear.Linear('Generator.Out', FC_DIM, cfg.OUTPUT_DIM, out))


def _conv_critic(inputs, groups, act, bn, stdev):
    """DCGANDiscriminator :435-467 (act 'lrelu' / 'tanh') and MultiplicativeDCGANDiscriminator :375-399 (act 'gate'): four 5x5 stride-2
    convs, BatchNorm in front of the nonlinearity of the last three, Linear -> D [n]."""
    dim = cfg.DIM
    m = 2 if act == 'gate' else 1
    if stdev:
        _stdev(True)
    try:
        out = inputs.reshape(-1, 3, 64, 64)
        out = _conv2d.Conv2D('Discriminator.1', 3, dim * m, 5, out, stride=2)
        out = _hidden(None, out, act, False, groups)
        for i, (ci, co) in ((2, (1, 2)), (3, (2, 4)), (4, (4, 8))):
            out = _conv2d.Conv2D('Discriminator.%d' % i, ci * dim, co * dim * m, 5, out, stride=2)
            out = _hidden('Discriminator.BN%d' % i, out, act, bn, groups)
        out = F.to_nchw(out).reshape(-1, 4 * 4 * 8 * dim)
        out = _linear.Linear('Discriminator.Output', 4 * 4 * 8 * dim, 1, out)
    finally:
        if stdev:
            _stdev(False)
    return out.reshape(-1)


def _g(act, bn=True, width=(8, 4, 2, 1), stdev=True):
    return lambda noise, groups: _deconv_generator(noise, groups, act, bn, width, stdev)


def _d(act, bn=True, stdev=True):
    return lambda inputs, groups: _conv_critic(inputs, groups, act, bn, stdev)


# ARCH -> (generator(noise, groups), critic(inputs, groups)); set_weights_stdev(0.02) wraps the DCGAN generator and critic only
ARCH_NETS = {
    'dcgan': (_g('relu'), _d('lrelu')),                                                          # :51
    'wganpaper': (_g('relu', bn=False, width=(1, 1, 1, 1), stdev=False), _d('lrelu')),   # :54
    'fc': (FCGenerator, _d('lrelu')),                                                            # :57
    'dcgan-nobn': (_g('relu', bn=False), _d('lrelu', bn=False)),                                 # :60
    'multiplicative': (_g('gate', stdev=False), _d('gate', stdev=False)),                        # :63
    'dcgan-tanh': (_g('tanh'), _d('tanh')),                                                      # :66-67
}


def train(next_batch, dev_batches=None, dev_every=200, **kw):
    """The training loop of TF/CT_gan_64x64.py:628-669 (dev cost and sample grid every 200 iterations, :660-665) on the caller's feeds:
    `next_batch()` -> int32 [BATCH_SIZE, 3*64*64] on the device, `dev_batches()` -> an iterable over the held-out batches."""
    import sys

    from . import dcgan_step
    kw.setdefault('sample_every', dev_every)
    return dcgan_step.train(sys.modules[__name__], next_batch, dev_batches, dev_every=dev_every, **kw)
