"""fp64 reference of the projection head (NOT in the reference scripts; Miyato & Koyama 2018): D(x, y) = f(x) . (w_out + E[y]) + b_out with
f = mean_hw relu(dropout(block 4)), the pooled feature the CT term reads as D_.  Plain torch, autograd for every gradient.  A helper module: no
fixtures, no marks.

Two levels:
  * head level - the six `ctgan_*_proj` launches of csrc/loss.hip as forward-only functions of (z, mask, w_out, b_out, E, labels), after
    tests/loss_heads_cases.py's ref_* (whose loss formulas are reused as they are);
  * step level - oracle/steps.py's resnet_d_losses / resnet_g_losses restated with the projected D: no ACGAN term, no clean pass, the CT term's D_
    still the plain feature, the rows [real, fake, real'] and x_hat of sample i all under labels[i].
"""
import torch

from oracle import nets, steps
from tests import loss_heads_cases as C

TABLE = 'Discriminator.Projection.W'


# ------------------------------------------------------------------------------------------------------------------ head level
def heads(y, w_out, b_out, emb, row_labels):
    """-> (f [n,nf], d [n]): d = f . (w_out + E[label]) + b_out, one label per row"""
    f = y.mean(dim=(2, 3))
    d = (f * (w_out.reshape(1, -1) + emb[row_labels.long()])).sum(dim=1) + (b_out if b_out is not None else 0.0)
    return f, d


def critic_heads(z, mask, w_out, b_out, emb, labels, B, lam2, M, gp):
    """rows [real, fake, real'] of B samples, row r under labels[r % B] -> ((cost, wgan, ct, 0, wgan + ct + gp), f, d, ct_i)"""
    f, d = heads(torch.relu(z) * mask, w_out, b_out, emb, labels.repeat(3))
    outs, ct_i = C.ref_critic_heads(d, f, None, labels, B, lam2, M, 0.0, gp)
    return outs, f, d, ct_i


def gen_heads(z, mask, w_out, b_out, emb, labels):
    """-> (cost = -mean(d), d)"""
    _, d = heads(torch.relu(z) * mask, w_out, b_out, emb, labels)
    return -d.mean(), d


def gp_seed(z, mask, w_out, emb, labels, create_graph=False):
    """dD/dz of the penalty rows (z must require grad): the sum over rows of D, whose rows do not interact"""
    _, d = heads(torch.relu(z) * mask, w_out, None, emb, labels)
    (gz,) = torch.autograd.grad(d.sum(), z, create_graph=create_graph)
    return gz


# ------------------------------------------------------------------------------------------------------------------ step level
def projected(reg, d, f, labels):
    return d + (f * reg[TABLE][labels.long()]).sum(dim=1)


def critic(reg, cfg, x, labels, kp1, kp2, kp3, u):
    d, f, _ = nets.resnet_discriminator(reg, cfg, x, labels, kp1, kp2, kp3, u)
    return projected(reg, d, f, labels), f


def d_losses(reg, cfg, real_int, labels, rnd, B, LAMBDA_2=2.0, Factor_M=0.0, GP_LAMBDA=10.0):
    """oracle.steps.resnet_d_losses with the projected critic (cfg: CONDITIONAL, not ACGAN)"""
    h = B // 2
    lab = [labels[:h], labels[h:]]
    with torch.no_grad():
        fake = torch.cat([nets.resnet_generator(reg, cfg, h, lab[i], rnd['z'][i]) for i in range(2)], 0)
    real = steps.resnet_real_prep(real_int, rnd['dequant'])
    rf = torch.cat([real, fake], 0)
    rf_labels = torch.cat([labels, labels], 0)
    d1, f1 = critic(reg, cfg, rf, rf_labels, 0.8, 0.5, 0.5, rnd['u_pass1'])
    d2, f2 = critic(reg, cfg, rf, rf_labels, 0.8, 0.5, 0.5, rnd['u_pass2'])
    wgan = d1[B:].mean() - d1[:B].mean()
    interp = (real + rnd['alpha'] * (fake - real)).detach().requires_grad_(True)
    dgp, _ = critic(reg, cfg, interp, labels, 0.8, 0.5, 0.5, rnd['u_gp'])
    grads = torch.autograd.grad(dgp.sum(), interp, create_graph=True)[0]
    slopes = torch.sqrt((grads ** 2).sum(dim=1))
    gp = GP_LAMBDA * ((slopes - 1.) ** 2).mean()
    ct = steps.ct_term(d1[:B], d2[:B], f1[:B], f2[:B], LAMBDA_2, Factor_M)
    cost = wgan + ct + gp
    return dict(cost=cost, wgan=cost, wgan_only=wgan, ct=ct, gp=gp, slopes=slopes, fake=fake, real=real, d_real=d1[:B], d_fake=d1[B:],
                gp_grads=grads)


def g_losses(reg, cfg, rnd, B, GEN_BS_MULTIPLE=2):
    """oracle.steps.resnet_g_losses with the projected critic: -mean D(G(z, y), y) over both towers"""
    n = GEN_BS_MULTIPLE * B // 2
    costs, samples = [], []
    for t in range(2):
        fake_labels = (rnd['label_u'][t] * 10).to(torch.int32)
        x = nets.resnet_generator(reg, cfg, n, fake_labels, rnd['z'][t])
        d, _ = critic(reg, cfg, x, fake_labels, 0.8, 0.5, 0.5, rnd['u'][t])
        costs.append(-d.mean())
        samples.append(x)
    return {'cost': sum(costs) / 2, 'samples': samples}


def grads_of(reg, cost, prefix):
    """{name: d cost / d parameter} over the trainable parameters whose name contains `prefix` (unused ones left out)"""
    named = list(reg.trainable_with_name(prefix))
    gs = torch.autograd.grad(cost, [p for _, p in named], allow_unused=True)
    return {n: g for (n, _), g in zip(named, gs) if g is not None}
