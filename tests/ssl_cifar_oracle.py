"""Torch restatement (fp64 by default, autograd) of the convolutional semi-supervised CT classifier - TH/CT_CIFAR.py with the parts of
TH/nn.py it uses (TH/ = CT-GANs/Theano_classifier of the reference) - IN THEANO'S GEOMETRY: `conv2d(padding=1|0, stride)` on
[out,in,k,k] filters and `conv_transpose2d(stride=2, padding=2, output_padding=1)` on [in,out,5,5] filters, images in the reference's
orientation.  Plus CPU stand-ins of the kernel wrappers ctgan_amd.kernels gained for it, so that the host logic of ctgan_amd.ct_cifar
runs without a GPU.  TEST INFRASTRUCTURE ONLY.

The product runs the same network on TF-SAME kernels in coordinates rotated by 180 degrees (ctgan_amd/ct_cifar.py, "Rotated
coordinates"); `relabel` / `unrelabel` are the parameter mapping stated there, `load_into_registry` applies it.  The oracle reads its
random numbers from oracle/philox.py by the stream ids and element positions documented in that docstring.  Written from the
scripts' mathematics, cited by line; nothing of their text is reused.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import philox
from tests.ssl_oracle import _rel_l2, _step_of, adam_theano, golden_matches, log_sum_exp, softplus, update_ok  # noqa: F401

SID_AUG_LAB, SID_AUG_UNL = 16, 17
EPS = 1e-6
N_CONV = 7          # layers 1..7 are 3x3 convs, 8 and 9 NIN, 10 dense


# ------------------------------------------------------------------------------------------------------------ streams
def uniforms(seed, sid, step, rows, cols, dtype=torch.float64):
    return torch.from_numpy(philox.uniform(seed, sid, step, rows * cols).reshape(rows, cols).copy()).to(dtype)


def dropout_mult(seed, sid, step, shape, keep, dtype=torch.float64):
    """The multiplier floor(keep + u) / keep of a dropout site over a logical [N, C, H, W] tensor in the reference's orientation: the
    kernels draw by the physical index of the channels-last ROTATED tensor, so position (n, c, h, w) takes value
    ((n H + (H-1-h)) W + (W-1-w)) C + c of the stream; keep + u is formed in fp32 as on the device."""
    N, C, H, W = shape
    u = philox.uniform(seed, sid, step, N * H * W * C).reshape(N, H, W, C)
    kept = np.floor(np.float32(keep) + u).astype(np.float64)
    m = torch.from_numpy(np.ascontiguousarray(kept.transpose(0, 3, 1, 2)[:, :, ::-1, ::-1]))
    return (m / float(np.float32(keep))).to(dtype)


# ------------------------------------------------------------------------------------------------------------ the project's SAME ops
def same_pads(size, k, stride):
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return total // 2, total - total // 2


def conv_same(x, w_hwio, stride=1):
    """This project's conv: TF 'SAME' cross-correlation with an HWIO filter (ctgan_amd.functional.conv2d)."""
    R, S = w_hwio.shape[:2]
    (pt, pb), (pl, pr) = same_pads(x.shape[2], R, stride), same_pads(x.shape[3], S, stride)
    return TF.conv2d(TF.pad(x, (pl, pr, pt, pb)), w_hwio.permute(3, 2, 0, 1), stride=stride)


def deconv_same(z, w_kkoi, stride=2):
    """This project's transposed conv (ctgan_amd.functional.conv2d_transpose): the data gradient of conv_same with the HWIO filter
    w_kkoi (I = out, O = in) on an input of `stride` times the size."""
    x = torch.zeros(z.shape[0], w_kkoi.shape[2], z.shape[2] * stride, z.shape[3] * stride, dtype=z.dtype, requires_grad=True)
    with torch.enable_grad():
        y = conv_same(x, w_kkoi, stride)
        (gx,) = torch.autograd.grad(y, x, z, create_graph=z.requires_grad or w_kkoi.requires_grad)
    return gx


def rot(x):
    return torch.flip(x, (2, 3))


# ------------------------------------------------------------------------------------------------------------ pieces
def lrelu(x, a=0.2):
    return torch.where(x > 0, x, a * x)


def wn_conv_weight(W, g, eps=EPS):
    """TH/nn.py:75-81: conv W [out,in,k,k], norm over (1,2,3)."""
    return W * (g / torch.sqrt(eps + (W * W).sum(dim=(1, 2, 3))))[:, None, None, None]


def wn_deconv_weight(W, g, eps=EPS):
    """TH/nn.py:71-73, :81: Deconv W [in,out,k,k], norm over (0,2,3) - per OUTPUT channel."""
    return W * (g / torch.sqrt(eps + (W * W).sum(dim=(0, 2, 3))))[None, :, None, None]


def wn_dense_weight(W, g, eps=EPS):
    return W * (g / torch.sqrt(eps + (W * W).sum(dim=0)))[None, :]


def wn_mid_weight(theta, s, eps):
    """The product's layout: theta [k,k,out,in], norm over (0,1,3)."""
    return theta * (s / torch.sqrt(eps + (theta * theta).sum(dim=(0, 1, 3))))[None, None, :, None]


def wn_mid_grad_formula(gW, theta, s, eps):
    """Closed form: d_o = sum gW theta, gs_o = d_o r_o, gtheta = s r (gW - theta d r^2) per output channel o."""
    r = 1.0 / torch.sqrt(eps + (theta * theta).sum(dim=(0, 1, 3)))
    d = (gW * theta).sum(dim=(0, 1, 3))
    bc = lambda v: v[None, None, :, None]          # noqa: E731
    return bc(s * r) * (gW - theta * bc(d * r * r)), d * r


def feat_match_l1(f, B):
    """TH/CT_CIFAR.py:152-156"""
    return (f[:B].mean(dim=0) - f[B:].mean(dim=0)).abs().mean()


def feat_match_l1_grad(f, B):
    d = f[:B].mean(dim=0) - f[B:].mean(dim=0)
    g = (torch.sign(d) / (f.shape[1] * B))[None, :].expand(B, -1)
    return torch.cat([g, -g], 0)


def batch_norm(a, b, axes):
    """TH/nn.py:194-216 with batch statistics, eps 1e-6 inside the root, offset b, no gain."""
    c = a - a.mean(dim=axes, keepdim=True)
    shape = [1, -1] + [1] * (a.dim() - 2)
    return c / torch.sqrt(1e-6 + (c * c).mean(dim=axes, keepdim=True)) + b.view(shape)


def _wn_post(P, n, a, init, init_stdv, pre):
    """TH/nn.py:85-95 on the pre-activation a ([n,c,h,w] or [n,c]): the init pass centres, scales and REPLACES P's g and b."""
    axes = (0, 2, 3) if a.dim() == 4 else (0,)
    shape = [1, -1] + [1] * (a.dim() - 2)
    if init:
        m = a.mean(dim=axes)
        a = a - m.view(shape)
        inv = init_stdv / torch.sqrt((a * a).mean(dim=axes))
        a = a * inv.view(shape)
        P[n + '.b'] = -m * inv
        P[n + '.g'] = P[n + '.g'] * inv
        if pre is not None:
            pre.append(a)
        return a
    return a + P[n + '.b'].view(shape)


# ------------------------------------------------------------------------------------------------------------ parameters
def d_names(cfg):
    names = []
    for l in range(1, 11):
        names += ['Classifier.%d.W' % l, 'Classifier.%d.g' % l, 'Classifier.%d.b' % l]
    return names, [n for n in names if not n.endswith('.g') or n == 'Classifier.10.g']


def g_names(cfg):
    n = []
    for i in (1, 2, 3):
        n += ['Generator.%d.W' % i, 'Generator.%d.bn_b' % i]
    return n + ['Generator.4.W', 'Generator.4.g', 'Generator.4.b']


def make_params(cfg, seed=0, dtype=torch.float64):
    """Fresh parameters in the script's distributions (N(0, 0.05) weights, unit g, zero b), in THEANO'S layouts."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.05          # noqa: E731
    P = collections.OrderedDict()
    s0, gw = cfg.IMG // 8, cfg.G_WIDTHS
    P['Generator.1.W'] = rn(cfg.Z_DIM, gw[0] * s0 * s0)
    P['Generator.1.bn_b'] = torch.zeros(gw[0] * s0 * s0, dtype=torch.float64)
    for i in (1, 2):
        P['Generator.%d.W' % (i + 1)] = rn(gw[i - 1], gw[i], 5, 5)
        P['Generator.%d.bn_b' % (i + 1)] = torch.zeros(gw[i], dtype=torch.float64)
    P['Generator.4.W'] = rn(gw[2], cfg.CHANNELS, 5, 5)
    P['Generator.4.g'] = torch.ones(cfg.CHANNELS, dtype=torch.float64)
    P['Generator.4.b'] = torch.zeros(cfg.CHANNELS, dtype=torch.float64)
    width = cfg.CHANNELS
    for l, w in enumerate(list(cfg.D_WIDTHS) + [cfg.N_CLASSES]):
        n = 'Classifier.%d' % (l + 1)
        P[n + '.W'] = rn(w, width, 3, 3) if l < N_CONV else rn(width, w)
        P[n + '.g'] = torch.ones(w, dtype=torch.float64)
        P[n + '.b'] = torch.zeros(w, dtype=torch.float64)
        width = w
    return collections.OrderedDict((n, v.to(dtype)) for n, v in P.items())


def relabel(name, v, cfg):
    """A parameter (or its gradient) in Theano's layout -> the product's registry layout (rotated coordinates)."""
    if name.startswith('Generator.1.'):
        s0 = cfg.IMG // 8
        return torch.flip(v.reshape(v.shape[:-1] + (cfg.G_WIDTHS[0], s0, s0)), (-2, -1)).reshape(v.shape)
    if v.dim() == 4:                       # conv [out,in,k,k] -> [k,k,in,out]; deconv [in,out,k,k] -> [k,k,out,in]
        return torch.flip(v, (2, 3)).permute(2, 3, 1, 0).contiguous()
    return v


def unrelabel(name, v, cfg):
    if name.startswith('Generator.1.'):
        return relabel(name, v, cfg)
    if v.dim() == 4:
        return torch.flip(v.permute(3, 2, 0, 1), (2, 3)).contiguous()
    return v


def load_into_registry(P, cfg=None):
    """Oracle parameters (Theano layouts) -> the product's registry (fp32, rotated filters in the project's layouts)."""
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    cfg = cfg or M.cfg
    lib.load_state_dict(collections.OrderedDict((n, relabel(n, v.detach(), cfg).to(torch.float32)) for n, v in P.items()), strict=True)


def from_registry(cfg=None, dtype=torch.float64):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    cfg = cfg or M.cfg
    return collections.OrderedDict((n, unrelabel(n, p.detach().cpu(), cfg).to(dtype)) for n, p in lib._params.items())


# ------------------------------------------------------------------------------------------------------------ networks
def generator(P, cfg, z, init=False, pre=None):
    """TH/CT_CIFAR.py:69-77 -> [B, 3, IMG, IMG] in the reference's orientation."""
    B, s0, gw = z.shape[0], cfg.IMG // 8, cfg.G_WIDTHS
    h = torch.relu(batch_norm(z @ P['Generator.1.W'], P['Generator.1.bn_b'], (0,))).view(B, gw[0], s0, s0)
    for i in (2, 3):
        a = TF.conv_transpose2d(h, P['Generator.%d.W' % i], stride=2, padding=2, output_padding=1)
        h = torch.relu(batch_norm(a, P['Generator.%d.bn_b' % i], (0, 2, 3)))
    a = TF.conv_transpose2d(h, wn_deconv_weight(P['Generator.4.W'], P['Generator.4.g']), stride=2, padding=2, output_padding=1)
    return torch.tanh(_wn_post(P, 'Generator.4', a, init, cfg.G_INIT_STDV, pre))


def classifier(P, cfg, x, masks=None, features=False, init=False, pre=None):
    """TH/CT_CIFAR.py:79-93.  masks: the three dropout multipliers (input, after layer 3, after layer 6), None: deterministic.
    features: False -> logits, True -> pooled features, 'both' -> (logits, features)."""
    h = x if masks is None else x * masks[0]
    for l in range(1, N_CONV + 1):
        n = 'Classifier.%d' % l
        a = TF.conv2d(h, wn_conv_weight(P[n + '.W'], P[n + '.g']), stride=2 if l in (3, 6) else 1, padding=0 if l == 7 else 1)
        h = lrelu(_wn_post(P, n, a, init, 1.0, pre))
        if masks is not None and l in (3, 6):
            h = h * masks[l // 3]
    for l in (8, 9):
        n = 'Classifier.%d' % l
        a = torch.einsum('nchw,co->nohw', h, wn_dense_weight(P[n + '.W'], P[n + '.g']))
        h = lrelu(_wn_post(P, n, a, init, 1.0, pre))
    feat = h.mean(dim=(2, 3))
    if features is True:
        return feat
    logits = _wn_post(P, 'Classifier.10', feat @ wn_dense_weight(P['Classifier.10.W'], P['Classifier.10.g']), init, cfg.D_INIT_STDV, pre)
    return (logits, feat) if features == 'both' else logits


def site_masks(cfg, seed, step, n, size, first_sid, dtype):
    w = cfg.D_WIDTHS
    shapes = [(n, cfg.CHANNELS, size, size), (n, w[2], size // 2, size // 2), (n, w[5], size // 4, size // 4)]
    keeps = [1.0 - cfg.DROP_IN, 1.0 - cfg.DROP_HIDDEN, 1.0 - cfg.DROP_HIDDEN]
    return [dropout_mult(seed, first_sid + k, step, s, kp, dtype) for k, (s, kp) in enumerate(zip(shapes, keeps))]


def init_passes(P, cfg, x_init, seed, step, pre=None):
    """:101-103, :205: the generator's init pass (one step of the counter, z at site 0), then the classifier's with dropout on (the
    next step, sites 0..2) over the padded init rows.  P's g and b are replaced."""
    dtype = x_init.dtype
    with torch.no_grad():
        generator(P, cfg, uniforms(seed, 0, step, cfg.BATCH_SIZE, cfg.Z_DIM, dtype), init=True, pre=pre)
        classifier(P, cfg, x_init, site_masks(cfg, seed, step + 1, x_init.shape[0], x_init.shape[2], 0, dtype), init=True, pre=pre)
    return P


def d_losses(P, cfg, x_lab, labels, x_unl, seed, step):
    """:105-128 on one stacked batch [lab ; unl ; unl ; fake]."""
    dtype, B = x_lab.dtype, x_lab.shape[0]
    with torch.no_grad():
        fake = generator(P, cfg, uniforms(seed, 0, step, B, cfg.Z_DIM, dtype))
    x_all = torch.cat([x_lab, x_unl, x_unl, fake], 0)
    logits, feat = classifier(P, cfg, x_all, site_masks(cfg, seed, step, 4 * B, x_all.shape[2], 1, dtype), features='both')
    lab, unl, unl2, fk = logits[:B], logits[B:2 * B], logits[2 * B:3 * B], logits[3 * B:]
    idx = labels.long()
    loss_lab = -lab[torch.arange(B), idx].mean() + log_sum_exp(lab).mean()
    loss_comp = ((torch.softmax(unl, 1) - torch.softmax(unl2, 1)) ** 2).mean()
    loss_feat = ((feat[B:2 * B] - feat[2 * B:3 * B]) ** 2).mean()
    l_unl = log_sum_exp(unl)
    loss_unl = (cfg.FEAT_WEIGHT * loss_feat + 0.5 * loss_comp - 0.5 * l_unl.mean() + 0.5 * softplus(l_unl).mean()
                + 0.5 * softplus(log_sum_exp(fk)).mean())
    train_err = (lab.argmax(dim=1) != idx).to(dtype).mean()
    train_err2 = (lab.max(dim=1).values <= 0).to(dtype).mean()
    return {'loss_lab': loss_lab, 'loss_unl': loss_unl, 'loss_comp': loss_comp, 'loss_feat': loss_feat, 'train_err': train_err,
            'train_err2': train_err2, 'logits': logits, 'cost': loss_lab + cfg.UNLABELED_WEIGHT * loss_unl}


def g_losses(P, cfg, x_unl, seed, step):
    """:152-156: features of a noisy pass over [G(z) ; x]."""
    dtype, B = x_unl.dtype, x_unl.shape[0]
    fake = generator(P, cfg, uniforms(seed, 0, step, B, cfg.Z_DIM, dtype))
    x_all = torch.cat([fake, x_unl], 0)
    f = classifier(P, cfg, x_all, site_masks(cfg, seed, step, 2 * B, x_all.shape[2], 1, dtype), features=True)
    return {'loss_gen': feat_match_l1(f, B)}


def _with_grad(P, names):
    Q = collections.OrderedDict((n, v.detach().clone()) for n, v in P.items())
    for n in names:
        Q[n].requires_grad_(True)
    return Q


def d_grads(P, cfg, x_lab, labels, x_unl, seed, step):
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
    """Parameters (Theano layouts), both Adam states, the averages and the stream position of a run of the oracle."""

    def __init__(self, P, cfg, seed, dtype=torch.float64):
        self.P = collections.OrderedDict((n, v.detach().clone().to(dtype)) for n, v in P.items())
        self.cfg, self.seed, self.step, self.dtype = cfg, seed, 0, dtype
        self.dn, self.gn = d_names(cfg)[1], g_names(cfg)
        z = lambda names: {n: torch.zeros_like(self.P[n]) for n in names}          # noqa: E731
        self.m, self.v, self.avg = z(self.dn + self.gn), z(self.dn + self.gn), z(self.dn)
        self.t = {'d': 1, 'g': 1}

    def init(self, x_init, pre=None):
        init_passes(self.P, self.cfg, x_init.to(self.dtype), self.seed, self.step, pre)
        self.step += 2

    def _apply(self, names, grads, which):
        c = self.cfg
        for n in names:
            self.P[n], self.m[n], self.v[n] = adam_theano(self.P[n], grads[n], self.m[n], self.v[n], self.t[which], c.LR, c.BETA1, c.BETA2)
            if which == 'd':
                self.avg[n] = self.avg[n] + c.AVG_RATE * (self.P[n] - self.avg[n])
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
        return float((self.predict(x, averaged).argmax(dim=1) != torch.as_tensor(y).long()).double().mean())


# ------------------------------------------------------------------------------------------------------------ gather reference
def byte_table():
    """The loader's expression (TH/cifar10_data.py, `unpickle`) on every byte value."""
    return np.asarray((-127.5 + np.arange(256, dtype=np.uint8)) / np.float32(255.0), dtype=np.float32)


def aug_draws(seed, sid, step, rows, pad):
    """(flip, oy, ox) per row: values 3r, 3r+1, 3r+2 of the uniform stream."""
    u = philox.uniform(int(seed), int(sid), int(step), 3 * rows).reshape(rows, 3)
    noff = 2 * pad + 1
    off = lambda v: np.minimum((np.float32(noff) * v).astype(np.int64), noff - 1)          # noqa: E731
    return u[:, 0] > np.float32(0.5), off(u[:, 1]), off(u[:, 2])


def gather_reference(data, idx, win, pad, draws=None, offset=None, flip=False):
    """numpy restatement of TH/CT_CIFAR.py:48, :211-222 -> float32 [rows, C, win, win] in the reference's orientation:
    np.pad(..., 'reflect'), the horizontal flip, the window, the loader's byte table.  draws: (flip, oy, ox) arrays per row, else the
    fixed `offset` (default: the unpadded image) and `flip`."""
    data, idx = np.asarray(data), np.asarray(idx)
    P = np.pad(data[idx], ((0, 0), (0, 0), (pad, pad), (pad, pad)), 'reflect') if pad else data[idx]
    rows = len(idx)
    if draws is None:
        oy, ox = (pad, pad) if offset is None else offset
        draws = (np.full(rows, bool(flip)), np.full(rows, oy), np.full(rows, ox))
    lut = byte_table()
    out = np.empty((rows, data.shape[1], win, win), dtype=np.float32)
    for r in range(rows):
        img = P[r][:, :, ::-1] if draws[0][r] else P[r]
        out[r] = lut[img[:, draws[1][r]:draws[1][r] + win, draws[2][r]:draws[2][r] + win]]
    return out


# ------------------------------------------------------------------------------------------------------------ CPU stand-ins
def _cl(t):
    out = torch.empty((t.shape[0], t.shape[2], t.shape[3], t.shape[1]), dtype=t.dtype).permute(0, 3, 1, 2)
    out.copy_(t)
    return out


def _wn_mid_fwd(theta, s, eps=0.0):
    rnorm = 1.0 / torch.sqrt(eps + (theta * theta).sum(dim=(0, 1, 3)))
    return theta * (s * rnorm)[None, None, :, None], rnorm


def _wn_mid_bwd(gw, theta, s, rnorm, want_gs=True):
    d = (gw * theta).sum(dim=(0, 1, 3))
    bc = lambda v: v[None, None, :, None]          # noqa: E731
    return bc(s * rnorm) * (gw - theta * bc(d * rnorm * rnorm)), (d * rnorm if want_gs else None)


def _wn_init_map(y, g, b, act=None, slope=0.2, init_stdv=1.0):
    axes = (0, 2, 3) if y.dim() == 4 else (0,)
    shape = [1, -1] + [1] * (y.dim() - 2)
    mean = y.mean(dim=axes)
    c = y - mean.view(shape)
    inv = init_stdv / torch.sqrt((c * c).mean(dim=axes))
    v = c * inv.view(shape)
    if act == 'lrelu':
        v = torch.where(v > 0, v, slope * v)
    elif act == 'tanh':
        v = torch.tanh(v)
    y.copy_(v)
    with torch.no_grad():
        g.copy_(g * inv)
        b.copy_(-mean * inv)
    return y


def _featcons_fwd(f, B, logits=None):
    d = f[B:2 * B] - f[2 * B:3 * B]
    err2 = (logits[:B].max(dim=1).values <= 0).float().mean() if logits is not None else torch.zeros(())
    return torch.stack([(d * d).mean(), err2])


def _featcons_bwd(f, gout, B):
    d = (f[B:2 * B] - f[2 * B:3 * B]) * (gout[0] * 2.0 / (B * f.shape[1]))
    z = torch.zeros_like(d)
    return torch.cat([z, d, -d, z], 0)


def _featmatch_l1_fwd(f, B):
    diff = f[:B].mean(dim=0) - f[B:].mean(dim=0)
    return diff.abs().mean(), diff


def _featmatch_l1_bwd(diff, gout, B):
    g = (gout * torch.sign(diff) / (diff.numel() * B))[None, :].expand(B, -1)
    return torch.cat([g, -g], 0)


def _aug_gather(data, idx, lut, win, pad, spec=None, offset=None, flip=False, rot180=True, channels_last=True, out=None):
    draws = None
    if spec is not None:
        seed, sid, ctr = spec
        draws = aug_draws(seed, sid, _step_of(ctr), idx.numel(), pad)
    res = gather_reference(data.numpy(), idx.numpy(), win, pad, draws, offset, flip)
    assert np.array_equal(lut.numpy(), byte_table())
    t = torch.from_numpy(np.ascontiguousarray(res[:, :, ::-1, ::-1]) if rot180 else res)
    t = _cl(t) if channels_last else t
    if out is not None:
        out.copy_(t)
        return out
    return t


def _bn_fwd_f64(x, scale, offset, labels, groups, relu, eps=1e-5):
    import ctgan_amd.kernels as K
    return K.bn_fwd(x, scale, offset, labels, groups, relu, eps)          # the cpu_kernels stand-in: no fp32 partial sums to avoid


STAND_INS = {'bn_fwd_f64': _bn_fwd_f64, 'wn_mid_fwd': _wn_mid_fwd, 'wn_mid_bwd': _wn_mid_bwd, 'wn_init_map': _wn_init_map, 'featcons_fwd': _featcons_fwd,
             'featcons_bwd': _featcons_bwd, 'featmatch_l1_fwd': _featmatch_l1_fwd, 'featmatch_l1_bwd': _featmatch_l1_bwd,
             'aug_gather': _aug_gather}


def install_stand_ins(monkeypatch):
    """Swap the wrappers of ctgan_amd.kernels the two semi-supervised modules added for CPU stand-ins (on top of `cpu_kernels`)."""
    import ctgan_amd.kernels as K
    from tests import ssl_oracle
    ssl_oracle.install_stand_ins(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(K, name, fn)


def small_cfg(**kw):
    """Reduced sizes for the host tests and the GPU step parity."""
    import ctgan_amd.ct_cifar as M
    d = dict(IMG=16, D_WIDTHS=(32, 32, 32, 64, 64, 64, 96, 64, 32), G_WIDTHS=(64, 32, 32), BATCH_SIZE=4, INIT_ROWS=12)
    d.update(kw)
    return M.configure(**d)


# ------------------------------------------------------------------------------------------------------------ step parity
def step_inputs(cfg, seed):
    """Images in the reference's orientation: (x_init padded [INIT_ROWS, 3, IMG + 2 PAD, ..], x_lab, x_unl, x_unl2, labels)."""
    g = torch.Generator().manual_seed(seed)
    B, S = cfg.BATCH_SIZE, cfg.IMG
    x_init = torch.rand(cfg.INIT_ROWS, cfg.CHANNELS, S + 2 * cfg.PAD, S + 2 * cfg.PAD, generator=g) - 0.5
    x_lab, x_unl, x_unl2 = (torch.rand(B, cfg.CHANNELS, S, S, generator=g) - 0.5 for _ in range(3))
    labels = torch.randint(0, cfg.N_CLASSES, (B,), generator=g, dtype=torch.int32)
    return x_init, x_lab, x_unl, x_unl2, labels


def _golden_init_names(cfg):
    return [n for n in d_names(cfg)[0] + g_names(cfg) if n.endswith(('.g', '.b')) and not n.endswith('.bn_b')]


def run_steps(dev, seed=5, cost_tol=2e-4, grad_tol=3e-3, log=None, golden=None):
    """The data-dependent init, one classifier step and one generator step of ctgan_amd.ct_cifar.CifarSSLTrainer (under the module's
    current Config, on `dev`) against the fp64 oracle on the same Philox streams, teacher-forced: before each step the product takes the
    oracle's weights.  Scalars within cost_tol * max(1, |ref|); every gradient within relative L2 max(grad_tol, 3 x the error of the
    fp32 twin of the oracle on the same inputs); updated parameters and averages by `update_ok`; only the step's trainable set moves.
    golden: a dict that receives the oracle's outputs.  Returns the number of parameters checked."""
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    cfg = M.cfg
    say = log or (lambda *a: None)
    x_init, x_lab, x_unl, x_unl2, labels = step_inputs(cfg, seed)
    to_dev = lambda x: M.rot180(x.to(dev))          # noqa: E731   (the internal form of a batch in the reference's orientation)
    lib.delete_all_params(); lib.set_seed(11)
    tr = M.CifarSSLTrainer(seed=seed)
    P = make_params(cfg, seed=seed, dtype=torch.float32)
    load_into_registry(P, cfg)
    st = State(P, cfg, seed)
    reg = lambda n: unrelabel(n, lib._params[n].detach().cpu(), cfg).double()          # noqa: E731
    checked = 0
    # ---- init
    tr.init_params(to_dev(x_init))
    st.init(x_init)
    for n in st.P:
        if n.endswith('.W') or n.endswith('.bn_b'):
            assert torch.equal(reg(n), P[n].double()), ('init moved', n)
        else:
            e = (reg(n) - st.P[n]).abs().max().item()
            say('init', n, 'max abs err', e)
            assert e <= 2e-4 * max(1.0, st.P[n].abs().max().item()), ('init', n, e)
    if golden is not None:
        golden.update({'init/' + n: st.P[n].numpy() for n in _golden_init_names(cfg)})
    assert int(tr.rng.ctr.item()) == st.step == 2
    avg_before = None
    for which in ('d', 'g'):
        lib.load_state_dict(collections.OrderedDict((n, relabel(n, v, cfg).float()) for n, v in st.P.items()), strict=True)
        before = {n: reg(n) for n in st.P}
        st.P = collections.OrderedDict((n, before[n].clone()) for n in st.P)       # the oracle continues from the fp32-rounded weights
        P32 = collections.OrderedDict((n, v.float()) for n, v in st.P.items())
        step = st.step
        if which == 'd':
            tr.d_opt.set_lr(cfg.LR)
            out, grads = tr.d_grads(to_dev(x_lab), labels.to(dev), to_dev(x_unl))
            tr.d_opt.update(grads, rng=tr.rng)
            ref, gref = st.d_step(x_lab, labels, x_unl)
            _, gtw = d_grads(P32, cfg, x_lab.float(), labels, x_unl.float(), seed, step)
            names, opt, keys = st.dn, tr.d_opt, ('loss_lab', 'loss_unl', 'loss_comp', 'loss_feat', 'train_err', 'train_err2')
        else:
            tr.g_opt.set_lr(cfg.LR)
            out, grads = tr.g_grads(to_dev(x_unl2))
            tr.g_opt.update(grads, rng=tr.rng)
            ref, gref = st.g_step(x_unl2)
            _, gtw = g_grads(P32, cfg, x_unl2.float(), seed, step)
            names, opt, keys = st.gn, tr.g_opt, ('loss_gen',)
        for k in keys:
            a, b = out[k].item(), ref[k].item()
            say(which, k, a, b)
            assert abs(a - b) <= cost_tol * max(1.0, abs(b)), (k, a, b)
            if golden is not None:
                golden['%s/%s' % (which, k)] = ref[k].numpy()
        assert [n for n, _ in (tr.d_named if which == 'd' else tr.g_named)] == names
        gp = {n: unrelabel(n, g.detach().cpu(), cfg) for n, g in zip(names, grads) if g is not None}
        for n in names:
            assert n in gp, ('no gradient', n)
            tol = max(grad_tol, 3 * _rel_l2(gtw[n], gref[n]))
            e = _rel_l2(gp[n], gref[n])
            say(which, 'grad', n, 'rel L2', e, 'bound', tol)
            assert (gp[n].double() - gref[n]).norm().item() <= tol * gref[n].norm().item() + 2e-6, (which, n, e, tol)
            if golden is not None and gref[n].numel() <= 512:
                golden['%s/grad/%s' % (which, n)] = gref[n].float().numpy()
        avgs = {n: unrelabel(n, a.detach().cpu(), cfg).double() for n, a in opt.avg_views()} if opt.avg is not None else {}
        for n in st.P:
            new = reg(n)
            if n not in names:
                assert torch.equal(new, before[n]), ('outside the trainable set, yet moved', which, n)
                continue
            ok, how = update_ok(new, before[n], st.P[n], gref[n], gp[n])
            say(which, 'update', n, how)
            assert ok, (which, 'update', n, how)
            if which == 'd':
                ok, how = update_ok(avgs[n], before[n], st.avg[n], gref[n], gp[n], scale=cfg.AVG_RATE)
                say(which, 'average', n, how)
                assert ok, (which, 'average', n, how)
            checked += 1
        if which == 'g':      # the generator step leaves the classifier's averages alone
            for n, a in tr.d_opt.avg_views():
                assert torch.equal(a.detach().cpu().double(), avg_before[n]), ('generator step moved an average', n)
        avg_before = {n: a.detach().cpu().double().clone() for n, a in tr.d_opt.avg_views()}
        assert int(tr.rng.ctr.item()) == st.step
    return checked


def oracle_golden(cfg, seed=5):
    """The oracle alone over the sequence run_steps drives - the weights rounded to fp32 between the steps as the teacher-forced
    product sees them - as the name -> array dict run_steps collects in `golden` (tests/golden/ssl_cifar_step.npz)."""
    x_init, x_lab, x_unl, x_unl2, labels = step_inputs(cfg, seed)
    st = State(make_params(cfg, seed=seed, dtype=torch.float32), cfg, seed)
    st.init(x_init)
    out = {'init/' + n: st.P[n].numpy() for n in _golden_init_names(cfg)}
    rnd = lambda: collections.OrderedDict((n, v.float().double()) for n, v in st.P.items())      # noqa: E731
    st.P = rnd()
    ref, gref = st.d_step(x_lab, labels, x_unl)
    out.update({'d/' + k: ref[k].numpy() for k in ('loss_lab', 'loss_unl', 'loss_comp', 'loss_feat', 'train_err', 'train_err2')})
    out.update({'d/grad/' + n: g.float().numpy() for n, g in gref.items() if g.numel() <= 512})
    st.P = rnd()
    ref, gref = st.g_step(x_unl2)
    out['g/loss_gen'] = ref['loss_gen'].numpy()
    out.update({'g/grad/' + n: g.float().numpy() for n, g in gref.items() if g.numel() <= 512})
    return out


# ------------------------------------------------------------------------------------------------------------ short loop
# Chosen on the CPU from the oracle alone (fp64, and its fp32 twin as a check that the outcome does not hang on rounding): with the script's
# dropout rates and init_stdv 0.1 on the logits a 150-iteration run at batch 20 either has not left loss_lab = log 10 or jumps between
# minima from iteration to iteration (fp64 and fp32 then end 0.4 apart); with the rates and learning rate below both descend smoothly
# and classify all 200 flat-colour test images (live-weight error 0.0 in fp64 and in fp32; about 12 s of fp64 oracle time).
LOOP_CFG = dict(IMG=16, D_WIDTHS=(16, 16, 16, 32, 32, 32, 32, 32, 16), G_WIDTHS=(16, 16, 16), BATCH_SIZE=20, INIT_ROWS=60, Z_DIM=8,
                LR=0.001, D_INIT_STDV=1.0, DROP_IN=0.05, DROP_HIDDEN=0.1)
LOOP_ITERS = 150


def synthetic_data(cfg, seed=0, n_train=400, n_test=200, count=10, spread=12.0):
    """Ten class-prototype uint8 images plus Gaussian pixel noise; `count` labelled examples per class (arrays for CifarSSLData).
    A prototype is one colour per class (a flat image, so that the flips and window offsets of the augmentation leave the class
    visible) from the corners and face centres of the colour cube."""
    r = np.random.RandomState(seed)
    cols = np.array([(a, b, c) for a in (56, 200) for b in (56, 200) for c in (56, 200)] + [(128, 128, 56), (128, 128, 200)], dtype=np.float64)
    proto = np.broadcast_to(cols[:cfg.N_CLASSES, :, None, None], (cfg.N_CLASSES, cfg.CHANNELS, cfg.IMG, cfg.IMG))

    def draw(n):
        y = np.arange(n) % cfg.N_CLASSES
        r.shuffle(y)
        x = np.clip(np.rint(proto[y] + spread * r.randn(n, cfg.CHANNELS, cfg.IMG, cfg.IMG)), 0, 255).astype(np.uint8)
        return x, y.astype(np.int32)
    (xt, yt), (xs, ys) = draw(n_train), draw(n_test)
    return {'x_train': xt, 'y_train': yt, 'x_test': xs, 'y_test': ys, 'count': count}


def loop_batches(cfg, data, iters, seed=1):
    """[(i_lab, labels, i_unl, i_unl2)] index batches of `iters` iterations through ctgan_amd.ct_cifar.CifarSSLData's epoch streams,
    and the init rows."""
    import ctgan_amd.ct_cifar as M
    d = M.CifarSSLData(arrays=data, count=data['count'], seed=seed, seed_data=seed)
    out, init_idx = [], None
    while len(out) < iters:
        n = d.begin_epoch()
        if init_idx is None:
            init_idx = d.init_indices().copy()
        for t in range(n):
            if len(out) < iters:
                out.append(tuple(np.ascontiguousarray(a) for a in d.batch(t)))
    return init_idx, out


def loop_oracle(cfg, data, init_idx, batches, seed=3, dtype=torch.float64):
    """The oracle over the loop, its batches made by gather_reference from the documented augmentation streams
    -> (live-weight test error, averaged-weight test error, [loss_lab per iteration])."""
    st = State(make_params(cfg, seed=seed, dtype=torch.float32), cfg, seed, dtype)
    tx, S, pad = data['x_train'], cfg.IMG, cfg.PAD
    t = lambda a: torch.from_numpy(a).to(dtype)          # noqa: E731
    st.init(t(gather_reference(tx, init_idx, S + 2 * pad, pad, offset=(0, 0))))
    B, trace = cfg.BATCH_SIZE, []
    for i_lab, y, i_unl, i_unl2 in batches:
        x_lab = gather_reference(tx, i_lab, S, pad, aug_draws(seed, SID_AUG_LAB, st.step, B, pad))
        x_unl = gather_reference(tx, i_unl, S, pad, aug_draws(seed, SID_AUG_UNL, st.step, B, pad))
        out, _ = st.d_step(t(x_lab), torch.from_numpy(y), t(x_unl))
        trace.append(float(out['loss_lab']))
        x_unl2 = gather_reference(tx, i_unl2, S, pad, aug_draws(seed, SID_AUG_LAB, st.step, B, pad))
        st.g_step(t(x_unl2))
    xs = t(gather_reference(data['x_test'], np.arange(len(data['x_test'])), S, pad))
    return st.test_error(xs, data['y_test'], averaged=False), st.test_error(xs, data['y_test'], averaged=True), trace


def loop_product(cfg, data, init_idx, batches, dev, seed=3, graphed=False):
    """The product over the same loop, same weights and streams -> (live-weight, averaged-weight test error, [loss_lab])."""
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    tr = M.CifarSSLTrainer(seed=seed, data=data['x_train'])
    load_into_registry(make_params(cfg, seed=seed, dtype=torch.float32), cfg)
    idx = torch.from_numpy(np.ascontiguousarray(init_idx)).to(dev)
    tr.init_params(tr.gather_fixed(idx, cfg.IMG + 2 * cfg.PAD, (0, 0)))
    step = tr
    if graphed:
        from ctgan_amd.engine import GraphedCifarSSLTrainer
        step = GraphedCifarSSLTrainer(tr)
        assert step.graphed, step.graph_error
    trace = []
    for b in batches:
        args = [torch.from_numpy(a) for a in b]
        out = step.train_iteration(*args) if graphed else tr.train_iteration_idx(*[a.to(dev) for a in args])
        trace.append(out['loss_lab'].clone())
    trace = [float(v) for v in torch.stack(trace).cpu()]
    bs = len(data['y_test'])
    return (tr.test_error(data['x_test'], data['y_test'], averaged=False, batch_size=bs),
            tr.test_error(data['x_test'], data['y_test'], batch_size=bs), trace)
