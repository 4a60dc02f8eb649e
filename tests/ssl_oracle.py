"""Torch restatement (fp64 by default, autograd) of the semi-supervised CT classifier - TH/CT_MNIST.py with the parts of TH/nn.py it
uses (TH/ = CT-GANs/Theano_classifier of the reference) - and CPU stand-ins (fp32 torch) of the kernel wrappers ctgan_amd.kernels
gained for it, so that the host logic of ctgan_amd.ct_mnist runs without a GPU.  TEST INFRASTRUCTURE ONLY.

The oracle reads its random numbers from oracle/philox.py by the stream ids documented in ctgan_amd/ct_mnist.py: per step, site 0 is
z (uniform), site 1 the input noise over the stacked rows, sites 2.. the noise after the hidden layers; the init pass has no z and
starts at site 0.  Written from the scripts' mathematics, cited by line; nothing of their text is reused.
"""
import collections
import math

import numpy as np
import torch

from oracle import philox


# ------------------------------------------------------------------------------------------------------------ streams
def normals(seed, sid, step, rows, cols, dtype=torch.float64):
    return torch.from_numpy(philox.normal(seed, sid, step, rows * cols).reshape(rows, cols).copy()).to(dtype)


def uniforms(seed, sid, step, rows, cols, dtype=torch.float64):
    return torch.from_numpy(philox.uniform(seed, sid, step, rows * cols).reshape(rows, cols).copy()).to(dtype)


# ------------------------------------------------------------------------------------------------------------ pieces
def log_sum_exp(x):
    """TH/nn.py:26-28"""
    m = x.max(dim=1).values
    return m + torch.log(torch.exp(x - m[:, None]).sum(dim=1))


def softplus(t):
    return torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))


def wn_weight(theta, s, eps=0.0):
    """TH/nn.py:407 (eps 0), :263 (eps 1e-6): per-output-column norm."""
    return theta * (s / torch.sqrt(eps + (theta * theta).sum(dim=0)))[None, :]


def wn_grad_formula(gW, theta, s, eps=0.0):
    """The closed form of the weight-norm gradient: d_j = sum_i gW_ij theta_ij, gs_j = d_j r_j, gtheta = s r (gW - theta d r^2)."""
    r = 1.0 / torch.sqrt(eps + (theta * theta).sum(dim=0))
    d = (gW * theta).sum(dim=0)
    return (s * r)[None, :] * (gW - theta * (d * r * r)[None, :]), d * r


def adam_theano(p, g, m, v, t, lr, b1=0.5, b2=0.999):
    """TH/nn.py:30-47; t counts from 1.  -> (p, m, v)"""
    m = b1 * m + (1. - b1) * g
    v = b2 * v + (1. - b2) * g * g
    return p - lr * (m / (1. - b1 ** t)) / torch.sqrt(v / (1. - b2 ** t) + 1e-8), m, v


def d_names(cfg):
    """Registry names of the classifier: every layer's theta, weight_scale, b; trainable: theta, b, and the last weight_scale."""
    L = len(cfg.HIDDEN) + 1
    names = []
    for l in range(1, L + 1):
        names += ['Classifier.%d.theta' % l, 'Classifier.%d.weight_scale' % l, 'Classifier.%d.b' % l]
    trainable = [n for n in names if not n.endswith('.weight_scale') or n == 'Classifier.%d.weight_scale' % L]
    return names, trainable


def g_names(cfg):
    n = []
    for i in range(1, len(cfg.G_HIDDEN) + 1):
        n += ['Generator.%d.W' % i, 'Generator.%d.bn_b' % i]
    k = len(cfg.G_HIDDEN) + 1
    return n + ['Generator.%d.W' % k, 'Generator.%d.W_scale' % k, 'Generator.%d.b' % k]


def make_params(cfg, seed=0, dtype=torch.float64):
    """Fresh parameters in the script's distributions (values are the test's own: the reference's numpy replay is not reproducible)."""
    g = torch.Generator().manual_seed(seed)
    P = collections.OrderedDict()
    width = cfg.Z_DIM
    for i, w in enumerate(cfg.G_HIDDEN):
        lim = math.sqrt(6. / (width + w))
        P['Generator.%d.W' % (i + 1)] = (torch.rand(width, w, generator=g, dtype=torch.float64) * 2 - 1) * lim
        P['Generator.%d.bn_b' % (i + 1)] = torch.zeros(w, dtype=torch.float64)
        width = w
    k = len(cfg.G_HIDDEN) + 1
    lim = math.sqrt(6. / (width + cfg.IN_DIM))
    P['Generator.%d.W' % k] = (torch.rand(width, cfg.IN_DIM, generator=g, dtype=torch.float64) * 2 - 1) * lim
    P['Generator.%d.W_scale' % k] = torch.ones(cfg.IN_DIM, dtype=torch.float64)
    P['Generator.%d.b' % k] = torch.zeros(cfg.IN_DIM, dtype=torch.float64)
    width = cfg.IN_DIM
    for l, w in enumerate(list(cfg.HIDDEN) + [cfg.N_CLASSES]):
        P['Classifier.%d.theta' % (l + 1)] = torch.randn(width, w, generator=g, dtype=torch.float64) * 0.1
        P['Classifier.%d.weight_scale' % (l + 1)] = torch.ones(w, dtype=torch.float64)
        P['Classifier.%d.b' % (l + 1)] = torch.zeros(w, dtype=torch.float64)
        width = w
    return collections.OrderedDict((n, v.to(dtype)) for n, v in P.items())


# ------------------------------------------------------------------------------------------------------------ networks
def generator(P, cfg, z):
    """TH/CT_MNIST.py:33-38; batch norm TH/nn.py:194-216 with batch statistics, eps 1e-6 inside the root, offset, no gain."""
    h = z
    for i in range(1, len(cfg.G_HIDDEN) + 1):
        a = h @ P['Generator.%d.W' % i]
        c = a - a.mean(dim=0, keepdim=True)
        a = c / torch.sqrt(1e-6 + (c * c).mean(dim=0, keepdim=True)) + P['Generator.%d.bn_b' % i][None, :]
        h = softplus(a)
    k = len(cfg.G_HIDDEN) + 1
    W = wn_weight(P['Generator.%d.W' % k], P['Generator.%d.W_scale' % k], 1e-6)
    return torch.sigmoid(h @ W + P['Generator.%d.b' % k][None, :])


def classifier(P, cfg, x, noise=None, features=False, init=False, pre=None):
    """TH/CT_MNIST.py:41-53.  noise: list of UNIT normal tensors, one per noise site in order (input, after hidden 1..), None:
    deterministic.  features: the last hidden layer's ReLU output before its noise (:92-93).  init: the data-dependent pass of
    TH/nn.py:421-426 - P's weight_scale and b are REPLACED (not in place); `pre`, a list, receives each layer's normalised
    pre-activation."""
    h = x if noise is None else x + cfg.SIGMA_IN * noise[0]
    L = len(cfg.HIDDEN) + 1
    for l in range(1, L + 1):
        n = 'Classifier.%d' % l
        a = h @ wn_weight(P[n + '.theta'], P[n + '.weight_scale'])
        if init:
            ma = a.mean(dim=0)
            a = a - ma[None, :]
            stdv = torch.sqrt((a * a).mean(dim=0))
            a = a / stdv[None, :]
            P[n + '.weight_scale'] = P[n + '.weight_scale'] / stdv
            P[n + '.b'] = -ma / stdv
            if pre is not None:
                pre.append(a)
        else:
            a = a + P[n + '.b'][None, :]
        if l == L:
            return a
        a = torch.relu(a)
        if features and l == L - 1:
            return a
        h = a if noise is None else a + cfg.SIGMA_HIDDEN * noise[l]
    raise AssertionError


def _site_noise(cfg, seed, step, rows, first_sid, n_hidden, dtype):
    widths = [cfg.IN_DIM] + list(cfg.HIDDEN)[:n_hidden]
    return [normals(seed, first_sid + k, step, rows, w, dtype) for k, w in enumerate(widths)]


def init_pass(P, cfg, x, seed, step, pre=None):
    """init_param (:109, :137): noisy pass with init=True; sites 0..5."""
    dtype = x.dtype
    with torch.no_grad():
        classifier(P, cfg, x, _site_noise(cfg, seed, step, x.shape[0], 0, len(cfg.HIDDEN), dtype), init=True, pre=pre)
    return P


def d_losses(P, cfg, x_lab, labels, x_unl, seed, step):
    """:64-90.  One stacked batch [lab ; unl ; unl2 ; fake]: every row's noise is its own stream position."""
    dtype = x_lab.dtype
    B = x_lab.shape[0]
    with torch.no_grad():
        fake = generator(P, cfg, uniforms(seed, 0, step, B, cfg.Z_DIM, dtype))
    x_all = torch.cat([x_lab, x_unl, x_unl, fake], 0)
    logits = classifier(P, cfg, x_all, _site_noise(cfg, seed, step, 4 * B, 1, len(cfg.HIDDEN), dtype))
    lab, unl, unl2, fk = logits[:B], logits[B:2 * B], logits[2 * B:3 * B], logits[3 * B:]
    lab_idx = labels.long()
    loss_lab = -lab[torch.arange(B), lab_idx].mean() + log_sum_exp(lab).mean()
    ct_i = ((torch.softmax(unl, 1) - torch.softmax(unl2, 1)) ** 2).mean(dim=1)
    CT = torch.clamp(cfg.LAMBDA_2 * ct_i - cfg.Factor_M, min=0).mean()
    l_unl = log_sum_exp(unl)
    loss_unl = 0.5 * (CT - l_unl.mean() + softplus(l_unl).mean() + softplus(log_sum_exp(fk)).mean())
    train_err = (lab.argmax(dim=1) != lab_idx).to(dtype).mean()
    return {'loss_lab': loss_lab, 'loss_unl': loss_unl, 'ct': CT, 'train_err': train_err, 'ct_i': ct_i, 'logits': logits,
            'cost': loss_lab + cfg.UNLABELED_WEIGHT * loss_unl}


def g_losses(P, cfg, x_unl, seed, step):
    """:92-94: features of a noisy pass over [G(z) ; x]; sites 0 (z), 1 (input noise), 2.. (hidden 1..4)."""
    dtype = x_unl.dtype
    B = x_unl.shape[0]
    fake = generator(P, cfg, uniforms(seed, 0, step, B, cfg.Z_DIM, dtype))
    f = classifier(P, cfg, torch.cat([fake, x_unl], 0), _site_noise(cfg, seed, step, 2 * B, 1, len(cfg.HIDDEN) - 1, dtype), features=True)
    return {'loss_gen': ((f[:B].mean(dim=0) - f[B:].mean(dim=0)) ** 2).mean()}


def _with_grad(P, names):
    Q = collections.OrderedDict((n, v.detach().clone()) for n, v in P.items())
    for n in names:
        Q[n].requires_grad_(True)
    return Q


def d_grads(P, cfg, x_lab, labels, x_unl, seed, step):
    """-> (losses, {name: gradient of the cost} over the classifier's trainable set)"""
    names = d_names(cfg)[1]
    Q = _with_grad(P, names)
    out = d_losses(Q, cfg, x_lab, labels, x_unl, seed, step)
    grads = torch.autograd.grad(out['cost'], [Q[n] for n in names])
    return {k: v.detach() for k, v in out.items()}, dict(zip(names, grads))


def g_grads(P, cfg, x_unl, seed, step):
    names = g_names(cfg)
    Q = _with_grad(P, names)
    out = g_losses(Q, cfg, x_unl, seed, step)
    grads = torch.autograd.grad(out['loss_gen'], [Q[n] for n in names])
    return {k: v.detach() for k, v in out.items()}, dict(zip(names, grads))


class State:
    """Parameters, both Adam states, the averages and the stream position of a run of the oracle."""

    def __init__(self, P, cfg, seed, dtype=torch.float64):
        self.P = collections.OrderedDict((n, v.detach().clone().to(dtype)) for n, v in P.items())
        self.cfg, self.seed, self.step, self.dtype = cfg, seed, 0, dtype
        self.dn, self.gn = d_names(cfg)[1], g_names(cfg)
        z = lambda names: {n: torch.zeros_like(self.P[n]) for n in names}          # noqa: E731
        self.m, self.v, self.avg = z(self.dn + self.gn), z(self.dn + self.gn), z(self.dn)
        self.t = {'d': 1, 'g': 1}

    def init(self, x):
        init_pass(self.P, self.cfg, x.to(self.dtype), self.seed, self.step)
        self.step += 1

    def _apply(self, names, grads, which):
        for n in names:
            self.P[n], self.m[n], self.v[n] = adam_theano(self.P[n], grads[n], self.m[n], self.v[n], self.t[which], self.cfg.LR, self.cfg.BETA1,
                                                          self.cfg.BETA2)
            if which == 'd':
                self.avg[n] = self.avg[n] + self.cfg.AVG_RATE * (self.P[n] - self.avg[n])
        self.t[which] += 1
        self.step += 1

    def d_step(self, x_lab, labels, x_unl):
        out, grads = d_grads(self.P, self.cfg, x_lab.to(self.dtype), labels, x_unl.to(self.dtype), self.seed, self.step)
        self._apply(self.dn, grads, 'd')
        return out, grads

    def g_step(self, x_unl):
        out, grads = g_grads(self.P, self.cfg, x_unl.to(self.dtype), self.seed, self.step)
        self._apply(self.gn, grads, 'g')
        return out, grads

    def predict(self, x, averaged=True):
        Q = dict(self.P)
        if averaged:
            Q.update(self.avg)
        with torch.no_grad():
            return classifier(Q, self.cfg, x.to(self.dtype))

    def test_error(self, x, y, averaged=True):
        return float((self.predict(x, averaged).argmax(dim=1) != y.long()).double().mean())


# ------------------------------------------------------------------------------------------------------------ CPU stand-ins
def _step_of(ctr):
    return int(ctr.reshape(-1)[0]) if torch.is_tensor(ctr) else int(ctr or 0)


def _wn_fwd(theta, s, eps=0.0):
    rnorm = 1.0 / torch.sqrt(eps + (theta * theta).sum(dim=0))
    return theta * (s * rnorm)[None, :], rnorm


def _wn_bwd(gw, theta, s, rnorm, want_gs=True):
    d = (gw * theta).sum(dim=0)
    return (s * rnorm)[None, :] * (gw - theta * (d * rnorm * rnorm)[None, :]), (d * rnorm if want_gs else None)


def _dense_noise_fwd(y, bias, relu, sigma, seed, stream_id, ctr, row_offset=0, want_a=False, out=None):
    a = y if bias is None else y + bias[None, :]
    if relu:
        a = torch.relu(a)
    h = a
    if sigma != 0:
        rows, cols = y.shape
        z = philox.normal(int(seed), int(stream_id), _step_of(ctr), (row_offset + rows) * cols)[row_offset * cols:]
        h = a + float(sigma) * torch.from_numpy(z.reshape(rows, cols).copy())
    if out is not None:
        out.copy_(h)
        h = out
    return h.clone() if h is y else h, (a.clone() if want_a else None)


def _dense_noise_bwd(gh, ga, y, bias, relu, want_gb=True):
    g = gh if ga is None else (ga if gh is None else gh + ga)
    if relu:
        pre = y if bias is None else y + bias[None, :]
        g = torch.where(pre > 0, g, torch.zeros_like(g))
    return g.clone(), (g.sum(dim=0) if want_gb else None)


def _wn_init(y, s, b, relu):
    mean = y.mean(dim=0)
    c = y - mean[None, :]
    stdv = torch.sqrt((c * c).mean(dim=0))
    v = c / stdv[None, :]
    y.copy_(torch.relu(v) if relu else v)
    with torch.no_grad():
        s.copy_(s / stdv)
        b.copy_(-mean / stdv)
    return y


def _head_terms(logits, labels, B, lam2, M):
    lab, unl, unl2, fk = logits[:B], logits[B:2 * B], logits[2 * B:3 * B], logits[3 * B:]
    idx = labels.long()
    loss_lab = -lab[torch.arange(B), idx].mean() + log_sum_exp(lab).mean()
    ct_i = ((torch.softmax(unl, 1) - torch.softmax(unl2, 1)) ** 2).mean(dim=1)
    CT = torch.clamp(lam2 * ct_i - M, min=0).mean()
    l_unl = log_sum_exp(unl)
    loss_unl = 0.5 * (CT - l_unl.mean() + softplus(l_unl).mean() + softplus(log_sum_exp(fk)).mean())
    err = (lab.argmax(dim=1) != idx).float().mean()
    return torch.stack([loss_lab, loss_unl, CT, err]), ct_i


def _ssl_head_fwd(logits, labels, B, lam2, M):
    out4, ct_i = _head_terms(logits.detach(), labels, B, lam2, M)
    return out4, ct_i


def _ssl_head_bwd(logits, labels, gout, B, lam2, M):
    x = logits.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        out4, _ = _head_terms(x, labels, B, lam2, M)
        (g,) = torch.autograd.grad(out4[0] * gout[0] + out4[1] * gout[1], x)
    return g


def _featmatch_fwd(f, B):
    diff = f[:B].mean(dim=0) - f[B:].mean(dim=0)
    return (diff * diff).mean(), diff


def _featmatch_bwd(diff, gout, B):
    g = (gout * 2.0 / (diff.numel() * B)) * diff[None, :].expand(B, -1)
    return torch.cat([g, -g], 0)


def _bn2d_fwd(x, offset, eps, act):
    c = x - x.mean(dim=0, keepdim=True)
    rstd = 1.0 / torch.sqrt(eps + (c * c).mean(dim=0))
    xhat = c * rstd[None, :]
    t = xhat if offset is None else xhat + offset[None, :]
    return (softplus(t) if act else t.clone()), xhat, rstd


def _bn2d_bwd(gy, xhat, offset, rstd, act, want_goffset=True):
    t = xhat if offset is None else xhat + offset[None, :]
    gt = gy * torch.sigmoid(t) if act else gy
    s1, s2 = gt.sum(dim=0), (gt * xhat).sum(dim=0)
    B = xhat.shape[0]
    gx = rstd[None, :] * (gt - s1[None, :] / B - xhat * s2[None, :] / B)
    return gx, (s1 if want_goffset else None)


def _adam_theano_step(theta, g, m, v, avg, state, beta1, beta2, eps=1e-8, avg_rate=0.0):
    lr, b1p, b2p = state[0].item(), state[1].item(), state[2].item()
    ok = torch.isfinite(g)
    state[3] += float((~ok).sum().item())
    gi = torch.where(ok, g, torch.zeros_like(g))
    m2 = beta1 * m + (1 - beta1) * gi
    v2 = beta2 * v + (1 - beta2) * gi * gi
    th2 = theta - lr * (m2 / (1 - b1p)) / torch.sqrt(v2 / (1 - b2p) + eps)
    m.copy_(torch.where(ok, m2, m)); v.copy_(torch.where(ok, v2, v)); theta.copy_(torch.where(ok, th2, theta))
    if avg is not None:
        avg.add_(avg_rate * (theta - avg))


STAND_INS = {'wn_fwd': _wn_fwd, 'wn_bwd': _wn_bwd, 'dense_noise_fwd': _dense_noise_fwd, 'dense_noise_bwd': _dense_noise_bwd,
             'wn_init': _wn_init, 'ssl_head_fwd': _ssl_head_fwd, 'ssl_head_bwd': _ssl_head_bwd, 'featmatch_fwd': _featmatch_fwd,
             'featmatch_bwd': _featmatch_bwd, 'bn2d_fwd': _bn2d_fwd, 'bn2d_bwd': _bn2d_bwd, 'adam_theano_step': _adam_theano_step}


def install_stand_ins(monkeypatch):
    """Swap the new wrappers of ctgan_amd.kernels for the stand-ins above (on top of the `cpu_kernels` fixture)."""
    import ctgan_amd.kernels as K
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(K, name, fn)


def small_cfg(**kw):
    """Reduced widths for host tests: the fp64 oracle runs in a fraction of a second."""
    import ctgan_amd.ct_mnist as M
    d = dict(IN_DIM=20, HIDDEN=(24, 16, 12, 12, 12), N_CLASSES=10, Z_DIM=8, G_HIDDEN=(16, 16), BATCH_SIZE=8, INIT_ROWS=40)
    d.update(kw)
    return M.configure(**d)


def load_into_registry(P):
    """Oracle parameters -> the product's registry (fp32)."""
    import ctgan_amd.tflib as lib
    lib.load_state_dict(collections.OrderedDict((n, v.detach().to(torch.float32)) for n, v in P.items()), strict=True)


# ------------------------------------------------------------------------------------------------------------ step parity
def update_ok(new, old, ref_new, g_ref, g_prod, tol=2e-2, scale=1.0):
    """The applied Adam update against the oracle's, in L2 - the rule of tests/test_gan_modes_host.py::_update_ok: within `tol` of the
    oracle's update plus the fp32 rounding of the weights themselves and 1e-9 per element; Adam's first step is ~ lr sign(g), so only
    elements whose gradient sign the product's fp32 gradient resolves (error below half the reference) are compared - the gradients
    themselves are checked separately.  scale: the same bound for a quantity that is `scale` times the parameter (the average after
    its first move from zero, scale = the averaging rate), plus that quantity's own fp32 rounding."""
    d, dr = (new - scale * old).reshape(-1), (ref_new - scale * old).reshape(-1)
    ulp = scale * (ref_new / scale).abs().reshape(-1) * 2.0 ** -23 + (0 if scale == 1.0 else ref_new.abs().reshape(-1) * 2.0 ** -23)
    gr, gp = g_ref.reshape(-1).double(), g_prod.detach().cpu().double().reshape(-1)
    keep = (gp - gr).abs() < 0.5 * gr.abs()
    d, dr, ulp = d[keep], dr[keep], ulp[keep]
    err = (d - dr).norm().item()
    return err <= tol * dr.norm().item() + ulp.norm().item() + 1e-9 * scale * d.numel() ** 0.5, (err, dr.norm().item(), ulp.norm().item())


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def step_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    B = cfg.BATCH_SIZE
    x_init = torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=g)
    x_lab, x_unl, x_unl2 = (torch.rand(B, cfg.IN_DIM, generator=g) for _ in range(3))
    labels = torch.randint(0, cfg.N_CLASSES, (B,), generator=g, dtype=torch.int32)
    return x_init, x_lab, x_unl, x_unl2, labels


def oracle_golden(cfg, seed=5):
    """The oracle alone over the sequence run_steps drives - init, one classifier step, one generator step from the inputs and weights
    of `seed`, the weights rounded to fp32 between the steps as the teacher-forced product sees them - as the name -> array dict
    run_steps collects in `golden` (tests/golden/ssl_step.npz)."""
    x_init, x_lab, x_unl, x_unl2, labels = step_inputs(cfg, seed)
    st = State(make_params(cfg, seed=seed, dtype=torch.float32), cfg, seed)
    st.init(x_init)
    out = {'init/' + n: st.P[n].numpy() for n in d_names(cfg)[0] if not n.endswith('.theta')}
    rnd = lambda: collections.OrderedDict((n, v.float().double()) for n, v in st.P.items())      # noqa: E731
    st.P = rnd()
    ref, gref = st.d_step(x_lab, labels, x_unl)
    out.update({'d/' + k: ref[k].numpy() for k in ('loss_lab', 'loss_unl', 'ct', 'train_err', 'ct_i')})
    out.update({'d/grad/' + n: g.float().numpy() for n, g in gref.items()})
    st.P = rnd()
    ref, gref = st.g_step(x_unl2)
    out['g/loss_gen'] = ref['loss_gen'].numpy()
    out.update({'g/grad/' + n: g.float().numpy() for n, g in gref.items()})
    return out


def golden_matches(got, want, tol=1e-6):
    """Every array of `got` equals the fixture's within tol * max(1, max |fixture|); the key sets are equal."""
    assert sorted(got) == sorted(want.files), (sorted(got), sorted(want.files))
    for k in want.files:
        a, b = np.asarray(got[k], dtype=np.float64), want[k].astype(np.float64)
        assert a.shape == b.shape and np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), k
    return len(want.files)


def run_steps(dev, seed=5, cost_tol=2e-4, grad_tol=3e-3, log=None, golden=None):
    """The data-dependent init, one classifier step and one generator step of ctgan_amd.ct_mnist.SSLTrainer (under the module's current
    Config, on `dev`) against the fp64 oracle on the same Philox streams, teacher-forced: before each step the product takes the oracle's
    weights.  Scalars and ct_i within cost_tol * max(1, |ref|); every gradient within relative L2 max(grad_tol, 3 x the error of the fp32
    twin of the oracle on the same inputs); updated parameters and averages by `update_ok`; only the step's trainable set moves.
    golden: a dict that receives the oracle's outputs (make_ssl_golden.py).  Returns the number of parameters checked."""
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    cfg = M.cfg
    say = log or (lambda *a: None)
    B = cfg.BATCH_SIZE
    x_init, x_lab, x_unl, x_unl2, labels = step_inputs(cfg, seed)
    lib.delete_all_params(); lib.set_seed(11)
    tr = M.SSLTrainer(seed=seed)
    P = make_params(cfg, seed=seed, dtype=torch.float32)
    load_into_registry(P)
    st = State(P, cfg, seed)
    reg = lambda n: lib._params[n].detach().cpu().double()          # noqa: E731
    tw = lambda t: t.float() if t.is_floating_point() else t        # noqa: E731
    checked = 0
    # ---- init
    tr.init_params(x_init.to(dev))
    st.init(x_init)
    for n in d_names(cfg)[0]:
        if n.endswith('.theta'):
            assert torch.equal(reg(n), P[n].double()), ('init moved a theta', n)
        else:
            e = (reg(n) - st.P[n]).abs().max().item()
            say('init', n, 'max abs err', e)
            assert e <= 2e-4 * max(1.0, st.P[n].abs().max().item()), ('init', n, e)
    if golden is not None:
        golden.update({'init/' + n: st.P[n].numpy() for n in d_names(cfg)[0] if not n.endswith('.theta')})
    assert int(tr.rng.ctr.item()) == st.step == 1
    for which in ('d', 'g'):
        lib.load_state_dict(collections.OrderedDict((n, v.float()) for n, v in st.P.items()), strict=True)
        before = {n: reg(n) for n in st.P}
        P64 = collections.OrderedDict((n, before[n].clone()) for n in st.P)       # the oracle continues from the fp32-rounded weights
        st.P = P64
        P32 = collections.OrderedDict((n, v.float()) for n, v in P64.items())
        step = st.step
        if which == 'd':
            tr.d_opt.set_lr(cfg.LR)
            out, grads = tr.d_grads(x_lab.to(dev), labels.to(dev), x_unl.to(dev))
            tr.d_opt.update(grads, rng=tr.rng)
            ref, gref = st.d_step(x_lab, labels, x_unl)
            _, gtw = d_grads(P32, cfg, x_lab, labels, x_unl, seed, step)
            names, opt = st.dn, tr.d_opt
            for k in ('loss_lab', 'loss_unl', 'ct', 'train_err'):
                a, b = out[k].item(), ref[k].item()
                say(which, k, a, b)
                assert abs(a - b) <= cost_tol * max(1.0, abs(b)), (k, a, b)
            e = (out['ct_i'].detach().cpu().double() - ref['ct_i']).abs().max().item()
            say(which, 'ct_i max abs err', e)
            assert e <= cost_tol, ('ct_i', e)
            if golden is not None:
                golden.update({'d/' + k: ref[k].numpy() for k in ('loss_lab', 'loss_unl', 'ct', 'train_err', 'ct_i')})
        else:
            tr.g_opt.set_lr(cfg.LR)
            out, grads = tr.g_grads(x_unl2.to(dev))
            tr.g_opt.update(grads, rng=tr.rng)
            ref, gref = st.g_step(x_unl2)
            _, gtw = g_grads(P32, cfg, x_unl2.float(), seed, step)
            names, opt = st.gn, tr.g_opt
            a, b = out['loss_gen'].item(), ref['loss_gen'].item()
            say(which, 'loss_gen', a, b)
            assert abs(a - b) <= cost_tol * max(1.0, abs(b)), ('loss_gen', a, b)
            if golden is not None:
                golden['g/loss_gen'] = ref['loss_gen'].numpy()
        assert [n for n, _ in (tr.d_named if which == 'd' else tr.g_named)] == names
        gp = dict(zip(names, grads))
        for n in names:
            assert gp[n] is not None, ('no gradient', n)
            tol = max(grad_tol, 3 * _rel_l2(gtw[n], gref[n]))
            e = _rel_l2(gp[n].detach().cpu(), gref[n])
            say(which, 'grad', n, 'rel L2', e, 'bound', tol)
            assert (gp[n].detach().cpu().double() - gref[n]).norm().item() <= tol * gref[n].norm().item() + 2e-6, (which, n, e, tol)
            if golden is not None:
                golden['%s/grad/%s' % (which, n)] = gref[n].float().numpy()
        avgs = dict(opt.avg_views()) if opt.avg is not None else {}
        for n in st.P:
            new = reg(n)
            if n not in names:
                assert torch.equal(new, before[n]), ('outside the trainable set, yet moved', which, n)
                continue
            ok, how = update_ok(new, before[n], st.P[n], gref[n], gp[n])
            say(which, 'update', n, how)
            assert ok, (which, 'update', n, how)
            if which == 'd':
                ok, how = update_ok(avgs[n].detach().cpu().double(), before[n], st.avg[n], gref[n], gp[n], scale=cfg.AVG_RATE)
                say(which, 'average', n, how)
                assert ok, (which, 'average', n, how)
            checked += 1
        if which == 'g':      # the generator step leaves the classifier's averages alone
            for n, a in tr.d_opt.avg_views():
                assert torch.equal(a.detach().cpu().double(), avg_before[n]), ('generator step moved an average', n)
        avg_before = {n: a.detach().cpu().double().clone() for n, a in tr.d_opt.avg_views()}
        assert int(tr.rng.ctr.item()) == st.step
    return checked


# ------------------------------------------------------------------------------------------------------------ short loop
LOOP_CFG = dict(IN_DIM=24, HIDDEN=(32, 24, 16, 16, 16), N_CLASSES=10, Z_DIM=8, G_HIDDEN=(16, 16), BATCH_SIZE=20, INIT_ROWS=100)


def synthetic_data(cfg, seed=0, n_train=400, n_test=200, count=10, spread=0.15):
    """Ten class prototypes in [0,1]^IN_DIM plus Gaussian noise, clipped to [0,1]; `count` labelled examples per class."""
    r = np.random.RandomState(seed)
    proto = r.rand(cfg.N_CLASSES, cfg.IN_DIM)

    def draw(n):
        y = np.arange(n) % cfg.N_CLASSES
        r.shuffle(y)
        return np.clip(proto[y] + spread * r.randn(n, cfg.IN_DIM), 0, 1).astype(np.float32), y.astype(np.int32)
    (xt, yt), (xs, ys) = draw(n_train), draw(n_test)
    lab = np.concatenate([np.where(yt == j)[0][:count] for j in range(cfg.N_CLASSES)])
    return {'x_train': xt, 'y_train': yt, 'x_lab': xt[lab], 'y_lab': yt[lab], 'x_test': xs, 'y_test': ys}


def loop_batches(cfg, data, iters, seed=1):
    """[(x_lab, labels, x_unl, x_unl2)] of `iters` iterations: labelled rows by permutations of the labelled set, the two unlabelled
    streams independent permutations of the training set (the epoch construction of TH/CT_MNIST.py:145-154 in miniature)."""
    r = np.random.RandomState(seed)
    B = cfg.BATCH_SIZE
    n_lab, n = len(data['x_lab']), len(data['x_train'])
    li = np.concatenate([r.permutation(n_lab) for _ in range(iters * B // n_lab + 1)])
    u1 = np.concatenate([r.permutation(n) for _ in range(iters * B // n + 1)])
    u2 = np.concatenate([r.permutation(n) for _ in range(iters * B // n + 1)])
    t = torch.from_numpy
    return [(t(data['x_lab'][li[i * B:(i + 1) * B]]), t(data['y_lab'][li[i * B:(i + 1) * B]]), t(data['x_train'][u1[i * B:(i + 1) * B]]),
             t(data['x_train'][u2[i * B:(i + 1) * B]])) for i in range(iters)]


def loop_oracle(cfg, data, batches, seed=3):
    """The fp64 oracle over the loop -> (live-weight test error, averaged-weight test error)."""
    st = State(make_params(cfg, seed=seed, dtype=torch.float32), cfg, seed)
    st.init(torch.from_numpy(data['x_train'][:cfg.INIT_ROWS]))
    for x_lab, y, x_unl, x_unl2 in batches:
        st.d_step(x_lab, y, x_unl)
        st.g_step(x_unl2)
    xs, ys = torch.from_numpy(data['x_test']), torch.from_numpy(data['y_test'])
    return st.test_error(xs, ys, averaged=False), st.test_error(xs, ys, averaged=True)


def loop_product(cfg, data, batches, dev, seed=3, graphed=False):
    """The product over the same loop, same weights and streams -> (live-weight, averaged-weight) test error."""
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    tr = M.SSLTrainer(seed=seed)
    load_into_registry(make_params(cfg, seed=seed, dtype=torch.float32))
    tr.init_params(torch.from_numpy(data['x_train'][:cfg.INIT_ROWS]).to(dev))
    step = tr
    if graphed:
        from ctgan_amd.engine import GraphedSSLTrainer
        step = GraphedSSLTrainer(tr)
        assert step.graphed, step.graph_error
    for x_lab, y, x_unl, x_unl2 in batches:
        if graphed:
            step.train_iteration(x_lab, y, x_unl, x_unl2)
        else:
            tr.train_iteration(x_lab.to(dev), y.to(dev), x_unl.to(dev), x_unl2.to(dev))
    bs = len(data['x_test'])
    return tr.test_error(data['x_test'], data['y_test'], averaged=False, batch_size=bs), tr.test_error(data['x_test'], data['y_test'], batch_size=bs)
