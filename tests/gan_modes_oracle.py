"""fp64 restatement of the scripts' other MODE branches (tests only): the batch-normalised nets of MODE 'wgan' (MNIST) and of every
non-CT mode (64x64 critic), the three loss kinds, TF RMSProp and the weight clip.  Built on oracle.tflib_ref / oracle.tf_ops; each function
names the reference lines it restates (TF = tensorflow_generative_model).

Two TF 1.x behaviours the reference tree relies on but does not contain are restated here: tf.train.RMSPropOptimizer's defaults (decay
0.9, momentum 0, epsilon 1e-10) and its `rms` slot, created at ONES; tf.nn.sigmoid_cross_entropy_with_logits' stable form."""
import torch

from oracle import nets as onets, tf_ops, tflib_ref as ops


# ----------------------------------------------------------------------------- nets
def mnist_generator(reg, n_samples, noise, DIM=64, bn=True, OUTPUT_DIM=784):
    """TF/CT_gan_mnist.py:62-87 with the MODE == 'wgan' batch norms (:67-68, :72-73, :79-80)."""
    if not bn:
        return onets.mnist_generator(reg, n_samples, noise, DIM=DIM)
    out = ops.Linear(reg, 'Generator.Input', 128, 4 * 4 * 4 * DIM, noise)
    out = torch.relu(ops.Batchnorm(reg, 'Generator.BN1', [0], out))
    out = out.reshape(-1, 4 * DIM, 4, 4)
    out = ops.Deconv2D(reg, 'Generator.2', 4 * DIM, 2 * DIM, 5, out)
    out = torch.relu(ops.Batchnorm(reg, 'Generator.BN2', [0, 2, 3], out))
    out = out[:, :, :7, :7]
    out = ops.Deconv2D(reg, 'Generator.3', 2 * DIM, DIM, 5, out)
    out = torch.relu(ops.Batchnorm(reg, 'Generator.BN3', [0, 2, 3], out))
    out = ops.Deconv2D(reg, 'Generator.5', DIM, 1, 5, out)
    return torch.sigmoid(out).reshape(-1, OUTPUT_DIM)


def mnist_discriminator(reg, inputs, u, DIM=64, bn=True):
    """TF/CT_gan_mnist.py:89-108 with the MODE == 'wgan' batch norms after conv 2 / 3, before the LeakyReLU (:96-97, :101-102)."""
    if not bn:
        return onets.mnist_discriminator(reg, inputs, u, DIM=DIM)
    out = inputs.reshape(-1, 1, 28, 28)
    out = ops.Conv2D(reg, 'Discriminator.1', 1, DIM, 5, out, stride=2)
    out = tf_ops.dropout(tf_ops.leaky_relu(out), 0.5, u[0])
    out = ops.Conv2D(reg, 'Discriminator.2', DIM, 2 * DIM, 5, out, stride=2)
    out = tf_ops.dropout(tf_ops.leaky_relu(ops.Batchnorm(reg, 'Discriminator.BN2', [0, 2, 3], out)), 0.5, u[1])
    out = ops.Conv2D(reg, 'Discriminator.3', 2 * DIM, 4 * DIM, 5, out, stride=2)
    out = tf_ops.dropout(tf_ops.leaky_relu(ops.Batchnorm(reg, 'Discriminator.BN3', [0, 2, 3], out)), 0.5, u[2])
    output2 = out.reshape(-1, 4 * 4 * 4 * DIM)
    out = ops.Linear(reg, 'Discriminator.Output', 4 * 4 * 4 * DIM, 1, output2)
    return out.reshape(-1), output2


def _g64_block_bn(reg, name, input_dim, output_dim, filter_size, x, resample):
    """TF/CT_gan_64x64.py:127-162 with Normalize = Batchnorm (MODE != 'wgan-ct', :87-92); only the critic's 'down' blocks."""
    assert resample == 'down'
    shortcut = ops.Conv2D(reg, name + '.Shortcut', input_dim, output_dim, 1, tf_ops.mean_pool2(x), he_init=False, biases=True)
    out = torch.relu(ops.Batchnorm(reg, name + '.BN1', [0, 2, 3], x, fused=True))
    out = ops.Conv2D(reg, name + '.Conv1', input_dim, input_dim, filter_size, out, biases=False)
    out = torch.relu(ops.Batchnorm(reg, name + '.BN2', [0, 2, 3], out, fused=True))
    out = tf_ops.mean_pool2(ops.Conv2D(reg, name + '.Conv2', input_dim, output_dim, filter_size, out))
    return shortcut + out


def good_discriminator_bn(reg, inputs, u, dim=64, kp=(0.8, 0.5, 0.5)):
    """GoodDiscriminator TF/CT_gan_64x64.py:357-373 with the BatchNorm critic of the non-CT modes."""
    out = inputs.reshape(-1, 3, 64, 64)
    out = ops.Conv2D(reg, 'Discriminator.Input', 3, dim, 3, out, he_init=False)
    out = _g64_block_bn(reg, 'Discriminator.Res1', dim, 2 * dim, 3, out, 'down')
    out = _g64_block_bn(reg, 'Discriminator.Res2', 2 * dim, 4 * dim, 3, out, 'down')
    out = tf_ops.dropout(out, kp[0], u[0])
    out = _g64_block_bn(reg, 'Discriminator.Res3', 4 * dim, 8 * dim, 3, out, 'down')
    out = tf_ops.dropout(out, kp[1], u[1])
    out = _g64_block_bn(reg, 'Discriminator.Res4', 8 * dim, 8 * dim, 3, out, 'down')
    out = tf_ops.dropout(out, kp[2], u[2])
    output2 = out.reshape(-1, 4 * 4 * 8 * dim)
    out = ops.Linear(reg, 'Discriminator.Output', 4 * 4 * 8 * dim, 1, output2)
    return out.reshape(-1), output2


# ----------------------------------------------------------------------------- losses
def bce_with_logits(x, z):
    """tf.nn.sigmoid_cross_entropy_with_logits(logits=x, labels=z) = max(x,0) - x z + log(1 + exp(-|x|)), elementwise.  TF/CT_gan_64x64.py
    :522-528 names the arguments; TF/CT_gan_mnist.py:181-195 passes them positionally (the meaning built here is the keyword one)."""
    return x.clamp_min(0) - x * z + torch.log1p(torch.exp(-x.abs()))


def d_cost(loss, d_real, d_fake):
    """disc_cost: 'wgan' TF/CT_gan_mnist.py:124, TF/CT_gan_64x64.py:494; 'bce' (MODE 'dcgan') TF/CT_gan_mnist.py:186-195,
    TF/CT_gan_64x64.py:524-533; 'ls' TF/CT_gan_64x64.py:537."""
    if loss == 'wgan':
        return d_fake.mean() - d_real.mean()
    if loss == 'bce':
        return (bce_with_logits(d_fake, torch.zeros_like(d_fake)).mean() + bce_with_logits(d_real, torch.ones_like(d_real)).mean()) / 2.
    if loss == 'ls':
        return (((d_real - 1) ** 2).mean() + ((d_fake - 0) ** 2).mean()) / 2.
    raise ValueError(loss)


def g_cost(loss, d_fake):
    """gen_cost: 'wgan' TF/CT_gan_mnist.py:123; 'bce' TF/CT_gan_mnist.py:181-184, TF/CT_gan_64x64.py:522-523; 'ls' TF/CT_gan_64x64.py:536."""
    if loss == 'wgan':
        return -d_fake.mean()
    if loss == 'bce':
        return bce_with_logits(d_fake, torch.ones_like(d_fake)).mean()
    if loss == 'ls':
        return ((d_fake - 1) ** 2).mean()
    raise ValueError(loss)


def d_losses(reg, G, D, real, rnd, loss):
    """The live critic calls of the non-CT branches: D(real) and D(fake), each its own call (own batch statistics, own dropout masks);
    TF prunes the other calls of TF/CT_gan_mnist.py:114-117 / TF/CT_gan_64x64.py:486-488 from these graphs."""
    B = real.shape[0]
    with torch.no_grad():
        fake = G(reg, B, rnd['z'])
    d_real, _ = D(reg, real, rnd['u_real'])
    d_fake, _ = D(reg, fake, rnd['u_fake'])
    return {'cost': d_cost(loss, d_real, d_fake), 'fake': fake, 'd_real': d_real, 'd_fake': d_fake}


def g_losses(reg, G, D, B, rnd, loss):
    x = G(reg, B, rnd['z'])
    d, _ = D(reg, x, rnd['u_fake'])
    return {'cost': g_cost(loss, d), 'samples': x}


# ----------------------------------------------------------------------------- optimizer, clip
def rmsprop_step(theta, g, ms, lr, rho=0.9, eps=1e-10):
    """tf.train.RMSPropOptimizer's ApplyRMSProp (momentum 0): ms += (g^2 - ms)(1 - rho); theta -= lr g / sqrt(ms + eps)."""
    ms = ms + (g * g - ms) * (1 - rho)
    return theta - lr * g / torch.sqrt(ms + eps), ms


class TFRMSProp:
    """tf.train.RMSPropOptimizer(learning_rate=lr) over a named parameter list (TF/CT_gan_mnist.py:125-131, TF/CT_gan_64x64.py:548-551,
    :572-575).  The `rms` slot starts at ones (TF 1.x's slot initialiser)."""

    def __init__(self, reg, names, lr, rho=0.9, eps=1e-10):
        self.reg, self.names, self.lr, self.rho, self.eps = reg, list(names), lr, rho, eps
        self.ms = {n: torch.ones_like(reg[n]).detach() for n in self.names}

    def apply(self, grads):
        with torch.no_grad():
            for n in self.names:
                g = grads.get(n)
                if g is None:
                    continue
                th, self.ms[n] = rmsprop_step(self.reg[n], g, self.ms[n], self.lr, self.rho, self.eps)
                self.reg[n].copy_(th)


def clip_critic(reg, bound=0.01):
    """clip_disc_weights: tf.clip_by_value over every lib.params_with_name('Discriminator') variable - the non-trainable moving statistics
    included (TF/CT_gan_mnist.py:134-143, TF/CT_gan_64x64.py:553-558)."""
    with torch.no_grad():
        for _, p in reg.params_with_name('Discriminator'):
            p.clamp_(-bound, bound)
