"""Case tables, fp64 references and the checks of the loss-head family (ctgan_amd/csrc/loss.hip), shared by tests/test_gpu_loss_paths.py (the HIP
kernels) and tests/test_loss_standins.py (their fp32 torch stand-ins in tests/cpu_kernels.py).  A plain helper module: no fixtures, no marks.

References: every operation is written once as a forward-only fp64 torch function (ref_*), after the comments of loss.hip and oracle/steps.py /
oracle/tf_ops.py; every gradient is torch.autograd.grad of that forward.  Two rules:
  * the hinge is torch.where(t >= 0, t, 0) with t = ct_i - M: its gradient at the tie t == 0 is 1, as TF's MaximumGrad and the kernels have it;
  * the gradient of the penalty for an all-zero row is 0 (the kernel's documented guard); autograd gives NaN there, that row is masked.
Input conditions are asserted on the reference (a test never hides behind an ill-posed input): slopes stay away from 1 (|s - 1| >= 0.25, or the
1e-6 bound on lambda * mean((s - 1)^2) would measure the cancellation in s - 1), no ct_i sits within 1e-4 (relative) of M except a crafted exact
tie, and the top-two logit gap is >= 1e-3 wherever an argmax is counted, except in a crafted tie of two equal maxima.

Bounds (the project's existing ones; none is derived from what the code under test returns):
  plain heads   (test_loss_heads)                     FWD_TOL 1e-6 on forward values, GRAD_TOL 1e-5 on gradients, in relerr = max-abs / max-abs;
                                                      1e-5 on mean_diff's value and on dot products over nf (d, a), as the existing tests have it
  fused scalars (test_fused_critic_[tail_]heads)      |got - ref| <= 2e-5 * max(1, |ref|)
  fused grads                                         ||got - ref|| <= 2e-5 ||ref|| + 1e-6 scale_all; gb_out, a sum that is analytically zero,
                                                      against the scale of the terms that cancel: 1e-6 * sum |gd|
  gan_loss      (test_gpu_gan_modes)                  value 1e-5 * max(1, |ref|); gradient rtol 1e-5, atol 1e-9
"""
import itertools
import math
import zlib

import torch

from oracle import tf_ops

FWD_TOL, GRAD_TOL, DOT_TOL = 1e-6, 1e-5, 1e-5
FUSED_TOL, FUSED_ABS = 2e-5, 1e-6
SENTINEL = 123.0

# largest error seen per kernel group in this process (printed by the test modules' teardown)
MEASURED = {}


def note(group, err):
    MEASURED[group] = max(MEASURED.get(group, 0.0), float(err))


def report():
    return '\n'.join('%-34s %.3g' % kv for kv in sorted(MEASURED.items()))


def f32(x):
    """x as the C ABI's float argument holds it."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 100000)


class Backend:
    """Where the code under test runs: K = ctgan_amd.kernels (HIP, or patched with the stand-ins), F = ctgan_amd.functional over the same K."""

    def __init__(self, K, F, device):
        self.K, self.F, self.device = K, F, device
        self.gpu = device != 'cpu'

    def dev(self, t):
        return t.detach().clone().contiguous().to(self.device)           # always a copy: some kernels update their argument in place

    def cl(self, t, extra_rows=0, fill=SENTINEL):
        """dense channels-last copy; extra_rows: the copy is the leading rows of a buffer whose other rows hold `fill` -> (view, buffer)"""
        n, c, h, w = t.shape
        buf = torch.full((n + extra_rows, h, w, c), fill, device=self.device, dtype=t.dtype).permute(0, 3, 1, 2)
        buf[:n].copy_(t.to(self.device))
        return (buf[:n], buf) if extra_rows else buf

    def off16(self, t):
        """the same values, contiguous, one float into a larger buffer: the data pointer is 4 past a 16-byte boundary"""
        buf = torch.zeros(t.numel() + 8, device=self.device, dtype=t.dtype)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t.to(self.device))
        assert not self.gpu or v.data_ptr() % 16 == 4
        return v

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize()


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def close(group, got, ref, tol):
    ref = torch.as_tensor(ref)
    assert tuple(got.shape) == tuple(ref.shape) or got.numel() == ref.numel() == 1, (group, got.shape, ref.shape)
    e = relerr(got.reshape(ref.shape), ref)
    note(group, e)
    assert e < tol, (group, e, tol)


def close_scalar(group, got, ref):
    got, ref = float(got.detach()), float(torch.as_tensor(ref).detach())
    e = abs(got - ref) / max(1.0, abs(ref))
    note(group, e)
    assert e < FUSED_TOL, (group, got, ref)


def close_l2(group, got, ref, scale):
    """||got - ref|| <= 2e-5 ||ref|| + 1e-6 scale; records the fraction of the bound used"""
    ref = ref.detach().double()
    diff = float((got.detach().cpu().double().reshape(ref.shape) - ref).norm())
    bound = FUSED_TOL * float(ref.norm()) + FUSED_ABS * float(scale)
    note(group + ' (of bound)', diff / bound if bound > 0 else (0.0 if diff == 0 else math.inf))
    assert diff <= bound, (group, diff, bound)


# ------------------------------------------------------------------------------------------------------------------ fp64 references (forward only)
def hinge(t):
    return torch.where(t >= 0, t, torch.zeros_like(t))


def ref_gp(g, lam):
    """:284-286  lambda * mean((||g_b|| - 1)^2) -> (gp, slopes)"""
    s = torch.sqrt((g * g).sum(dim=1))
    return lam * ((s - 1) ** 2).mean(), s


def ref_ct_rows(d, d_, f, f_, lam2):
    """:288-290, as oracle.steps.ct_term before its maximum"""
    return lam2 * (d - d_) ** 2 + lam2 * 0.1 * ((f - f_) ** 2).mean(dim=1)


def ref_ct(d, d_, f, f_, lam2, M):
    ct_i = ref_ct_rows(d, d_, f, f_, lam2)
    return hinge(ct_i - M).mean(), ct_i


def ref_ce(logits, labels):
    return tf_ops.sparse_softmax_ce(logits, labels).mean()           # log_softmax in the dtype of `logits`


def ref_mean_diff(x, na, nb, sa, sb):
    out = x.new_zeros(())
    if na:
        out = out + sa * x[:na].mean()
    if nb:
        out = out + sb * x[na:na + nb].mean()
    return out


def ref_critic_heads(d, f, a, labels, B, lam2, M, scale, gp):
    """-> (cost, wgan, ct, acgan, wgan + ct + gp), ct_i   (:244-248, :288-291)"""
    wgan = d[B:2 * B].mean() - d[:B].mean()
    ct_i = ref_ct_rows(d[:B], d[2 * B:], f[:B], f[2 * B:], lam2)
    ct = hinge(ct_i - M).mean()
    ac = ref_ce(a[:B], labels) if a is not None else torch.zeros((), dtype=d.dtype)
    pen = gp if gp is not None else 0.0
    return (wgan + ct + pen + scale * ac, wgan, ct, ac, wgan + ct + pen), ct_i


def ref_tail_heads(y, w_out, b_out, w_ac, b_ac, relu=False):
    """:179-186  f = mean_hw (relu) y, d = f . w_out + b_out, a = f . w_ac + b_ac"""
    f = (torch.relu(y) if relu else y).mean(dim=(2, 3))
    d = a = None
    if w_out is not None:
        d = f @ w_out.reshape(-1) + (b_out if b_out is not None else 0.0)
    if w_ac is not None:
        a = f @ w_ac + (b_ac if b_ac is not None else 0.0)
    return f, d, a


def ref_gen_heads(y, w_out, b_out, w_ac, b_ac, labels, scale):
    """:321-330  -mean(d) + scale * CE(a, labels)"""
    f, d, a = ref_tail_heads(y, w_out, b_out, w_ac, b_ac)
    cost = -d.mean()
    if a is not None:
        cost = cost + scale * ref_ce(a, labels)
    return cost, d, a


def ref_gp_finish(ga, gs, scale):
    v = ga + scale * tf_ops.upsample2(gs)
    return v, torch.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(dim=1))


def midpoint_M(ct_i):
    """M between the two middle values of the sorted ct_i (fp32-representable): half of the hinges on, half off"""
    s = ct_i.detach().sort().values
    k = s.numel() // 2
    return f32((s[k - 1] + s[k]) / 2)


def off_tie(ct_i, M, but=()):
    if M == 0.0:                                         # ct_i >= 0 in any precision: every hinge is on, and where ct_i == 0 its gradient is 0 too
        return True
    c = ct_i.detach()
    keep = torch.ones_like(c, dtype=torch.bool)
    for i in but:
        keep[i] = False
    return bool((((c - M).abs() / c.abs())[keep] >= 1e-4).all())


def seeded(make, tries=32):
    """make(trial) -> inputs, or None where they miss an input condition (two middle ct_i too close for a clean midpoint): the first trial
    that meets it, deterministically; the condition itself is asserted again by the caller"""
    for trial in range(tries):
        res = make(trial)
        if res is not None:
            return res
    raise AssertionError('no trial met the input condition')


def assert_off_tie(ct_i, M, but=()):
    assert off_tie(ct_i, M, but), 'a hinge sits on the tie'


def with_gap(logits, but=()):
    """fp32 logits whose top-two gap is >= 1e-3 in every row (a near-tie is pushed apart), except rows `but`; asserted on the fp64 values"""
    logits = logits.clone()
    if logits.shape[1] > 1:
        top = logits.topk(2, dim=1)
        near = (top.values[:, 0] - top.values[:, 1]) < 1e-2
        for i in but:
            near[i] = False
        logits[near, top.indices[near, 0]] += 0.05
        assert_gap(logits, but)
    return logits


def assert_gap(logits, but=()):
    if logits.shape[1] < 2:
        return
    top = logits.detach().double().topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    for i in but:
        gap[i] = 1.0
    assert (gap >= 1e-3).all(), 'an argmax is decided by less than 1e-3'


def make_tie(logits, row, k1, k2):
    """two equal maxima in `row` at columns k1 < k2 (exactly representable)"""
    logits[row] = logits[row].clamp(max=3.0)
    logits[row, k1] = logits[row, k2] = 8.0


# ------------------------------------------------------------------------------------------------------------------ gp_fwd / gp_bwd / gp_bwd_mean
# (B, d): one element; one pass of the row loop short of / past 256; batch loop past 256; B * d past 4096 blocks of 256 threads, where the
# grid-stride loops of gp_bwd_kernel / gp_bwd_mean_kernel start their second pass (a wrong stride can show at no smaller size)
GP_CASES = [(1, 1), (3, 255), (3, 257), (300, 7), (2, 600001)]
GP_TARGETS = (0.5, 2.0, 3.0, 1.6)


def gp_inputs(B, d, zero_row):
    x = torch.randn(B, d, generator=gen('gp', B, d), dtype=torch.float64)
    t = torch.tensor([GP_TARGETS[i % 4] for i in range(B)], dtype=torch.float64)
    x = (x / x.norm(dim=1, keepdim=True) * t[:, None]).float()
    if zero_row is not None:
        x[zero_row] = 0
    return x


def check_gp(be, B, d):
    K, lam, go = be.K, 10.0, f32(0.7)
    for zero_row in (None, B // 2):
        x = gp_inputs(B, d, zero_row)
        xr = x.double().requires_grad_(True)
        gp_ref, s_ref = ref_gp(xr, lam)
        live = s_ref.detach() > 0
        assert ((s_ref.detach()[live] - 1).abs() >= 0.25).all()
        (gref,) = torch.autograd.grad(gp_ref * go, xr)
        if zero_row is not None:
            assert torch.isnan(gref[zero_row]).all()           # autograd's sqrt' at 0; the kernel's guard gives 0
            gref = gref.clone(); gref[zero_row] = 0
        assert torch.isfinite(gref).all()
        gp_ref, s_ref = gp_ref.detach(), s_ref.detach()
        xd, gout = be.dev(x), be.dev(torch.tensor(go))
        gp, slopes = K.gp_fwd(xd, lam)
        close('gp fwd', slopes, s_ref, FWD_TOL); close('gp fwd', gp, gp_ref, FWD_TOL)
        gg = K.gp_bwd(xd, slopes, gout, lam)
        close('gp bwd', gg, gref, GRAD_TOL)
        if zero_row is not None:
            row = gg[zero_row].cpu()
            assert torch.isfinite(row).all() and (row == 0).all()
        _, slopes2 = K.gp_fwd(xd, lam, defer_mean=True)         # the mean is left to tail_critic_heads_fwd(slopes=...): check_tail_critic
        assert torch.equal(slopes2, slopes)
        gg2, gp2 = K.gp_bwd_mean(xd, slopes, gout, lam)
        assert torch.equal(gg2, gg)
        close('gp fwd', gp2, gp_ref, FWD_TOL)
        out5 = be.dev(torch.tensor([1.5, -2.25, 0.75, 3.0, -0.5]))
        before = out5.clone()
        gg3, gp3 = K.gp_bwd_mean(xd, slopes, gout, lam, out5=out5)
        assert torch.equal(gg3, gg) and torch.equal(gp3, gp2)
        assert torch.equal(out5[1:4], before[1:4])
        for k in (0, 4):
            close('gp fwd', out5[k], before[k].cpu().double() + gp_ref, FWD_TOL)


# ------------------------------------------------------------------------------------------------------------------ ct_fwd / ct_bwd
# (B, nf): batch loop past 256; feature loop short of / past 256; B * (nf + 1) past 4096 * 256, the second pass of ct_bwd_kernel's stride loop
CT_CASES = [(1, 1), (5, 3), (300, 130), (2, 1000), (2, 600000)]
CT_MS = ('zero', 'mid', 'tie')


def ct_inputs(key, B, nf, tie):
    g = gen(*key)
    d, d_ = torch.randn(B, generator=g), torch.randn(B, generator=g)
    f, f_ = torch.randn(B, nf, generator=g), torch.randn(B, nf, generator=g)
    if tie:                                              # row 0: d - d_ = 1, f == f_, lambda2 = 2 -> ct_i = 2 = M bitwise, in any precision
        d[0], d_[0] = 1.5, 0.5
        f_[0] = f[0]
    return d, d_, f, f_


def check_ct(be, B, nf, Mkind):
    if Mkind == 'mid' and B < 2:
        return
    K, lam2, go = be.K, 2.0, f32(1.3)
    tie = Mkind == 'tie'

    def make(trial):
        ins = ct_inputs(('ct', B, nf, trial), B, nf, tie)
        ct_i = ref_ct_rows(*[t.double() for t in ins], lam2)
        M = 2.0 if tie else (0.0 if Mkind == 'zero' else midpoint_M(ct_i))
        return (ins, M) if off_tie(ct_i, M, but=(0,) if tie else ()) else None
    ins, M = seeded(make)
    leaves = [t.double().requires_grad_(True) for t in ins]
    ct_i_ref = ref_ct_rows(*leaves, lam2).detach()
    assert_off_tie(ct_i_ref, M, but=(0,) if tie else ())
    if tie:
        assert ct_i_ref[0].item() == M
    ref, _ = ref_ct(*leaves, lam2, M)
    gref = torch.autograd.grad(ref * go, leaves)
    if tie:
        assert gref[0][0].item() == go * lam2 * 2 / B    # the tie's gradient goes to the first argument
    dv = [be.dev(t) for t in ins]
    ct, ct_i = K.ct_fwd(*dv, lam2, M)
    close('ct fwd', ct_i, ct_i_ref, FWD_TOL); close('ct fwd', ct, ref.detach(), FWD_TOL)
    if tie:
        assert ct_i[0].item() == M
    got = K.ct_bwd(*dv, ct_i, be.dev(torch.tensor(go)), lam2, M)
    for a, b in zip(got, gref):
        close('ct bwd', a, b, GRAD_TOL)


# ------------------------------------------------------------------------------------------------------------------ softmax_ce_fwd / softmax_ce_bwd
CE_CASES = [(1, 1), (7, 2), (300, 10), (5, 1000)]        # (B, ncls): the one-thread-per-row loop past 256
CE_KINDS = ('plain', 'big', 'tie')


def check_softmax_ce(be, B, ncls, kind):
    if kind == 'tie' and (B < 2 or ncls < 2):
        return
    K, go = be.K, 2.0
    g = gen('ce', B, ncls, kind)
    logits = torch.randn(B, ncls, generator=g) * 3
    labels = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
    ties = ()
    if kind == 'big':                                    # logits of magnitude 80: exp() of the raw values overflows fp32
        logits[::2, 0] = 80.0
        logits[1::2, 0] = -80.0
        if ncls > 1:
            logits[::2, -1] = -80.0
    logits = with_gap(logits)
    if kind == 'tie':                                    # the first of two equal maxima wins: row 0 is a hit, row 1 a miss
        make_tie(logits, 0, 0, ncls - 1); make_tie(logits, 1, 0, ncls - 1)
        labels[0], labels[1] = 0, ncls - 1
        ties = (0, 1)
        assert_gap(logits, but=ties)
    lr = logits.double().requires_grad_(True)
    ref = ref_ce(lr, labels)
    (gref,) = torch.autograd.grad(ref * go, lr)
    nc_ref = (logits.double().argmax(1) == labels.long()).sum().item()
    loss, probs, nc = K.softmax_ce_fwd(be.dev(logits), be.dev(labels))
    assert torch.isfinite(loss).item() and torch.isfinite(probs).all()
    close('softmax_ce fwd', loss, ref.detach(), FWD_TOL)
    assert nc.item() == nc_ref
    gl = K.softmax_ce_bwd(probs, be.dev(labels), be.dev(torch.tensor(go)))
    close('softmax_ce bwd', gl, gref, GRAD_TOL)


# ------------------------------------------------------------------------------------------------------------------ mean_diff_fwd / mean_diff_bwd
MEAN_DIFF_CASES = [(0, 5), (5, 0), (1, 1), (300, 7), (7, 300)]      # an empty half on either side; each half's loop past 256


def check_mean_diff(be, na, nb):
    K = be.K
    g = gen('md', na, nb)
    x = torch.cat([torch.randn(na, generator=g) + 2, torch.randn(nb, generator=g) - 1])     # the two means do not cancel
    for sa, sb in ((-1.0, 1.0), (f32(0.3), f32(-1.7))):
        xr = x.double().requires_grad_(True)
        ref = ref_mean_diff(xr, na, nb, sa, sb)
        (gref,) = torch.autograd.grad(ref * 2.0, xr)
        close('mean_diff fwd', K.mean_diff_fwd(be.dev(x), na, nb, sa, sb), ref.detach(), DOT_TOL)
        close('mean_diff bwd', K.mean_diff_bwd(be.dev(torch.tensor(2.0)), na, nb, sa, sb), gref, GRAD_TOL)


# ------------------------------------------------------------------------------------------------------------------ gan_loss_fwd / gan_loss_bwd
GAN_LOSS_CASES = [(loss, net, B) for loss in ('bce', 'ls') for net in ('d', 'g') for B in (1, 257)]


def check_gan_loss(be, loss, net, B):
    from tests import gan_modes_oracle as O
    K = be.K
    n = 2 * B if net == 'd' else B
    d = (torch.randn(n, generator=gen('gan', loss, net, B)) * 3).double()
    if B > 1:
        d[0], d[1], d[-1], d[-2] = 80.0, -80.0, 80.0, -80.0
    x = d.clone().requires_grad_(True)
    ref = O.d_cost(loss, x[:B], x[B:]) if net == 'd' else O.g_cost(loss, x)
    (gref,) = torch.autograd.grad(ref, x)
    kind = K.GAN_LOSS_KINDS[(loss, net)]
    dv = be.dev(d.float())
    out = K.gan_loss_fwd(dv, B, kind)
    gd = K.gan_loss_bwd(dv, be.dev(torch.tensor(0.75)), B, kind)
    assert torch.isfinite(out).item() and torch.isfinite(gd).all()
    e = abs(out.item() - ref.item()) / max(1.0, abs(ref.item()))
    note('gan_loss fwd', e)
    assert e <= 1e-5, (out.item(), ref.item())
    note('gan_loss bwd', relerr(gd, 0.75 * gref))
    assert torch.allclose(gd.cpu().double(), 0.75 * gref, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------------ accuracy2
ACC_CASES = [(1, 1, False), (5, 2, False), (200, 10, False), (5, 2, True), (200, 10, True)]      # (B, ncls, tie): 2B past 256


def acc_ref(logits, labels, B):
    am = logits.double().argmax(dim=1)
    lab = labels.long()
    return (am[:B] == lab).double().mean().item(), (am[B:] == lab).double().mean().item()


def check_accuracy2(be, B, ncls, tie):
    g = gen('acc', B, ncls, tie)
    logits = with_gap(torch.randn(2 * B, ncls, generator=g) * 3)
    labels = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
    if tie:                                              # real row 0: the label is the first maximum (hit); fake row 1: the second (miss)
        make_tie(logits, 0, 0, ncls - 1); make_tie(logits, B + 1, 0, ncls - 1)
        labels[0], labels[1] = 0, ncls - 1
        assert_gap(logits, but=(0, B + 1))
    ref = acc_ref(logits, labels, B)
    acc = be.K.accuracy2(be.dev(logits), be.dev(labels), B)
    for k in (0, 1):
        note('accuracy2', abs(acc[k].item() - ref[k]))
        assert abs(acc[k].item() - ref[k]) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ critic_heads_fwd / critic_heads_bwd
# (B, nf, ncls, f one float off a 16-byte boundary): narrow shapes (B > 256: every batch loop a second pass); then B * nf around 65536, the
# threshold of the one-workgroup-per-sample CT_i kernel: just under it, on it with float4 loads, past it with scalar loads (nf % 4), and on it with
# a misaligned f, which falls back to one wave per row; last, 3B * nf past 4096 * 256: the second pass of critic_heads_bwd_kernel's stride loop
CRITIC_HEADS_CASES = [(1, 1, 1, False), (5, 3, 2, False), (260, 8, 3, False),
                      (8, 8191, 10, False), (8, 8192, 10, False), (8, 8193, 10, False), (8, 8192, 10, True), (4, 98304, 10, False)]
HEAD_W = [0.3, -1.1, 0.6, 0.9]                           # weights of (cost, wgan, ct, acgan) for the n_gout = 4 gradient


def check_critic_heads(be, B, nf, ncls, misaligned):
    F = be.F
    lam2, scale0, gp0 = 2.0, f32(0.7), f32(0.37)
    Ms = ('zero', 'mid') if B > 1 else ('zero',)
    if (B, nf) in ((5, 3), (8, 8192)):
        Ms = Ms + ('tie',)
    combos = list(itertools.product((True, False), (True, False), Ms))
    if B * nf > (1 << 18):                               # the 4.7 MB case: its point is the backward's stride loop, two combinations reach it
        combos = [(True, True, 'mid'), (False, False, 'zero')]
    for with_a, with_gp, Mkind in combos:
        tie = Mkind == 'tie'

        def make(trial):
            g = gen('ch', B, nf, ncls, trial)
            d = torch.randn(3 * B, generator=g); f = torch.randn(3 * B, nf, generator=g); a = torch.randn(3 * B, ncls, generator=g) * 2
            lab = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
            if tie:
                d[0], d[2 * B] = 1.5, 0.5
                f[2 * B] = f[0]
            ct_i = ref_ct_rows(d[:B].double(), d[2 * B:].double(), f[:B].double(), f[2 * B:].double(), lam2)
            M = 2.0 if tie else (0.0 if Mkind == 'zero' else midpoint_M(ct_i))
            return (d, f, a, lab, M) if off_tie(ct_i, M, but=(0,) if tie else ()) else None
        d, f, a, lab, M = seeded(make)
        scale = scale0 if with_a else 0.0
        dr = d.double().requires_grad_(True); fr = f.double().requires_grad_(True); ar = a.double().requires_grad_(True)
        ct_i_ref = ref_ct_rows(dr[:B], dr[2 * B:], fr[:B], fr[2 * B:], lam2).detach()
        assert_off_tie(ct_i_ref, M, but=(0,) if tie else ())
        if tie:
            assert ct_i_ref[0].item() == M
        ref, _ = ref_critic_heads(dr, fr, ar if with_a else None, lab, B, lam2, M, scale, gp0 if with_gp else None)
        dd = be.dev(d).requires_grad_(True); ad = be.dev(a).requires_grad_(True)
        fd = (be.off16(f) if misaligned else be.dev(f)).requires_grad_(True)
        gpv = be.dev(torch.tensor(gp0)).requires_grad_(True) if with_gp else None
        got = F.critic_heads(dd, fd, ad if with_a else None, be.dev(lab), B, lam2, M, scale, gp=gpv)
        for x, y in zip(got, ref):
            close_scalar('critic_heads fwd', x, y)
        ins = [dd, fd] + ([ad] if with_a else []); rins = [dr, fr] + ([ar] if with_a else [])
        for w in ([1.0, 0.0, 0.0, 0.0], HEAD_W):         # n_gout = 1, then 4
            if w[0] == 1.0:
                comb, combr = got[0], ref[0]
            else:
                comb = sum(wi * gi for wi, gi in zip(w, got[:4])); combr = sum(wi * ri for wi, ri in zip(w, ref[:4]))
            gg = torch.autograd.grad(comb, ins + ([gpv] if with_gp else []), retain_graph=True)
            gr = torch.autograd.grad(combr, rins, retain_graph=True)
            scale_all = max(float(t.abs().max()) for t in gr)
            for x, y in zip(gg, gr):
                close_l2('critic_heads bwd', x, y, scale_all)
            if with_gp:
                assert abs(gg[-1].item() - w[0]) < 1e-6  # d cost / d gp = 1
            if Mkind == 'tie':
                assert float(gr[0][2 * B]) != 0.0        # the tie's hinge is on in the reference
        if Mkind == 'tie':
            _, ct_i, _ = be.K.critic_heads_fwd(dd.detach(), fd.detach(), None, None, B, lam2, M, 0.0)
            assert ct_i[0].item() == M
            close('critic_heads fwd ct_i', ct_i, ct_i_ref, FUSED_TOL)


# ------------------------------------------------------------------------------------------------------------------ tail_heads_fwd
# head_row slices its 256 threads as S = 256 / (nf / 4) position slices of nf / 4 channel quads:
#   nf      4    12    256   260   512   1020   1024
#   nf/4    1     3     64    65   128    255    256
#   S     256    85      4     3     2      1      1      idle threads: 1 (nf 12), 61 (260), 1 (1020)
# nf > 256: the j += 256 loops run again; hw < S: most slices stay empty (hw = 1: all but one); nout = (critic head) + ncls outputs over four waves
TAIL_NF = (4, 12, 256, 260, 512, 1020, 1024)
TAIL_HW = ((1, 1), (2, 2), (7, 7))
TAIL_HEADS = ('both', 'critic', 'class', 'neither')
# (n, nf, H, W, relu, heads, biases, ncls): the nf x hw product; the other axes cycle at different periods, so every value of every axis occurs
TAIL_FWD_CASES = [((1, 5)[(i // 3) % 2], nf, H, W, bool(i % 2), TAIL_HEADS[i % 4], i % 5 != 0, (1, 10, 13)[(i // 2) % 3])
                  for i, (nf, (H, W)) in enumerate(itertools.product(TAIL_NF, TAIL_HW))]


def head_params(g, nf, ncls):
    w_out = torch.randn(nf, 1, generator=g) * (2 / math.sqrt(nf)); b_out = torch.randn(1, generator=g)
    w_ac = torch.randn(nf, ncls, generator=g) * (2 / math.sqrt(nf)); b_ac = torch.randn(ncls, generator=g)
    return w_out, b_out, w_ac, b_ac


def check_tail_fwd(be, n, nf, H, W, relu, heads, biases, ncls):
    g = gen('tf', n, nf, H, W, relu, heads, biases, ncls)
    y = torch.randn(n, nf, H, W, generator=g)
    w_out, b_out, w_ac, b_ac = head_params(g, nf, ncls)
    if heads in ('class', 'neither'):
        w_out = b_out = None
    if heads in ('critic', 'neither'):
        w_ac = b_ac = None
    if not biases:
        b_out = b_ac = None
    opt = lambda t, fn: fn(t) if t is not None else None
    rf, rd, ra = ref_tail_heads(y.double(), *[opt(t, torch.Tensor.double) for t in (w_out, b_out, w_ac, b_ac)], relu=relu)
    f, d, a = be.K.tail_heads_fwd(be.cl(y), *[opt(t, be.dev) for t in (w_out, b_out, w_ac, b_ac)], relu=relu)
    close('tail_heads fwd f', f, rf, FWD_TOL)
    assert (d is None) == (rd is None) and (a is None) == (ra is None)
    if d is not None:
        close('tail_heads fwd d, a', d, rd, DOT_TOL)
    if a is not None:
        close('tail_heads fwd d, a', a, ra, DOT_TOL)


# ------------------------------------------------------------------------------------------------------------------ tail_critic_heads_fwd + tail_heads_bwd
# (B, nf, H, W, ncls).  tail_heads_bwd_kernel's dynamic shared memory holds max(nf, 3B) floats: 3B > nf in (5, 12), (90, 8), (260, 4); nf > 3B in the
# others.  3B > 256 (the gds fill's second pass) in (90, 8) and (260, 4); B > 256 (critic_heads_final's loops) in (260, 4).  The weight-gradient
# blocks take four outputs each, n_all = nf (1 + nac) + 1 + nac of them: n_all % 4 = 2, 2, 3, 3, 3, 3, 3, 0 with the class head, 1 without it.
TAIL_CRITIC_CASES = [(1, 4, 1, 1, 1), (5, 12, 2, 2, 13), (2, 260, 7, 7, 10), (90, 8, 1, 1, 10), (2, 1020, 1, 3, 10), (2, 1024, 7, 7, 10),
                     (3, 512, 3, 3, 10), (260, 4, 1, 1, 3)]


def masked_relu_inputs(g, rows, nf, H, W, keep):
    """z, mask: y = relu(z) * mask is what the last conv's epilogue writes (relu + dropout with 1/keep)"""
    z = torch.randn(rows, nf, H, W, generator=g)
    mask = (torch.rand(rows, nf, H, W, generator=g) < keep).float() / keep
    return z, mask


def clean_rows_with_gap(key, rows, nf, H, W, w_ac, b_ac, relu):
    """rows of the dropout-free pass whose class-head logits (fp64) have a top-two gap >= 1e-3 in every row: the first seed that has"""
    for s in range(64):
        yc = torch.randn(rows, nf, H, W, generator=gen(key, s))
        _, _, a = ref_tail_heads(yc.double(), None, None, w_ac.double(), b_ac.double(), relu=relu)
        top = a.topk(2, dim=1).values if a.shape[1] > 1 else None
        if top is None or ((top[:, 0] - top[:, 1]) >= 1e-3).all():
            return yc, a
    raise AssertionError('no seed with a clear argmax in every row')


def tail_critic_ref(zr, mask, P, lab, B, lam2, M, scale, gp, with_a):
    y = torch.relu(zr) * mask
    f, d, a = ref_tail_heads(y, P[0], P[1], P[2] if with_a else None, P[3] if with_a else None)
    outs, ct_i = ref_critic_heads(d, f, a, lab, B, lam2, M, scale, gp)
    return outs, f, d, a, ct_i


def check_tail_grads(group, got, ref, gd_ref):
    """(gy, gw_out, gb_out[, gw_ac, gb_ac]) against autograd; gb_out = sum gd is analytically 0: bounded against sum |gd|"""
    scale_all = max(float(t.abs().max()) for t in ref)
    for i, (x, y) in enumerate(zip(got, ref)):
        close_l2(group, x, y, float(gd_ref.abs().sum()) if i == 2 else scale_all)


def check_tail_critic(be, B, nf, H, W, ncls):
    K, F = be.K, be.F
    lam2, scale0, gp0, keep = 2.0, f32(0.7), f32(0.37), 0.5
    ms = 1.0 / keep

    def make(trial):
        g = gen('tc', B, nf, H, W, ncls, trial)
        z, mask = masked_relu_inputs(g, 3 * B, nf, H, W, keep)
        params = head_params(g, nf, ncls)
        lab = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
        ct_i0 = tail_critic_ref(z.double(), mask.double(), [t.double() for t in params], lab, B, lam2, 0.0, 0.0, None, False)[4]
        Ms = [0.0] + ([midpoint_M(ct_i0)] if B > 1 else [])
        return (g, z, mask, params, lab, Ms) if all(off_tie(ct_i0, M) for M in Ms) else None
    g, z, mask, params, lab, Ms = seeded(make)
    y = torch.relu(z) * mask
    zr = z.double().requires_grad_(True)
    P = [t.double().requires_grad_(True) for t in params]
    labd = be.dev(lab)
    for with_a, M in itertools.product((True, False), Ms):
        scale = scale0 if with_a else 0.0
        outs, fr, dr, ar, ct_i_ref = tail_critic_ref(zr, mask.double(), P, lab, B, lam2, M, scale, gp0, with_a)
        assert_off_tie(ct_i_ref, M)
        yd = be.cl(y).requires_grad_(True)
        Pd = [be.dev(t).requires_grad_(True) for t in params]
        gpv = be.dev(torch.tensor(gp0)).requires_grad_(True)
        got = F.critic_tail_heads(yd, Pd[0], Pd[1], Pd[2] if with_a else None, Pd[3] if with_a else None, labd, B, lam2, M, scale, ms, gp=gpv)
        for x, r in zip(got[:5], outs):
            close_scalar('tail_critic_heads fwd', x, r)
        close('tail_critic_heads fwd d', got[5], dr.detach(), DOT_TOL)
        ins = [yd, Pd[0], Pd[1]] + ([Pd[2], Pd[3]] if with_a else [])
        rins = [zr, P[0], P[1]] + ([P[2], P[3]] if with_a else [])
        for w in ([1.0, 0.0, 0.0, 0.0], HEAD_W):         # n_gout = 1, then 4
            if w[0] == 1.0:
                comb, combr = got[0], outs[0]
            else:
                comb = sum(wi * gi for wi, gi in zip(w, got[:4])); combr = sum(wi * ri for wi, ri in zip(w, outs[:4]))
            gg = torch.autograd.grad(comb, ins, retain_graph=True)
            gr = torch.autograd.grad(combr, rins + [dr], retain_graph=True)
            check_tail_grads('tail_heads bwd', gg, gr[:-1], gr[-1])

        # the same forward with the penalty's mean and the clean pass folded in (ctgan_tail_critic_heads_fwd with slopes / y_clean), then the backward with its
        # outputs in the leading rows of larger buffers and the penalty pass's rows riding the launch
        sl = torch.tensor([GP_TARGETS[i % 4] for i in range(B)]) + torch.rand(B, generator=g) * 0.1
        gp_ref = 10.0 * ((sl.double() - 1) ** 2).mean()
        for clean_relu in ((False, True) if with_a else (None,)):
            slot = be.dev(torch.full((1,), SENTINEL))
            yc = a_c_ref = None
            if clean_relu is not None:
                yc, a_c_ref = clean_rows_with_gap(('tc-clean', B, nf, H, W, clean_relu), 2 * B, nf, H, W, params[2], params[3], clean_relu)
            Pk = [be.dev(t) for t in params]
            out, f, d, a, ct_i, probs, acc = K.tail_critic_heads_fwd(
                be.cl(y), B, Pk[0], Pk[1], Pk[2] if with_a else None, Pk[3] if with_a else None, labd, slot, lam2, M, scale,
                slopes=be.dev(sl), gp_lambda=10.0, y_clean=be.cl(yc) if yc is not None else None, clean_relu=bool(clean_relu))
            close('tail_critic_heads fwd gp slot', slot, gp_ref.reshape(1), FWD_TOL)
            ref5 = [outs[0] - gp0 + gp_ref, outs[1], outs[2], outs[3], outs[4] - gp0 + gp_ref]
            for x, r in zip(out, ref5):
                close_scalar('tail_critic_heads fwd', x, r)
            close('tail_heads fwd f', f, fr.detach(), FWD_TOL)
            close('tail_critic_heads fwd d', d, dr.detach(), DOT_TOL)
            close('tail_critic_heads fwd ct_i', ct_i, ct_i_ref.detach(), FUSED_TOL)
            if with_a:
                close('tail_heads fwd d, a', a, ar.detach(), DOT_TOL)
                want = acc_ref(a_c_ref, lab, B)
                for k in (0, 1):
                    assert abs(acc[k].item() - want[k]) < 1e-6, (clean_relu, acc, want)
            else:
                assert a is None and probs is None and acc is None
        for n_gp, w in ((0, HEAD_W), (1, HEAD_W), (7, [f32(0.8)]), (7, HEAD_W)):
            gout = be.dev(torch.tensor(w))
            wr = w if len(w) == 4 else [w[0], 0.0, 0.0, 0.0]
            gr = torch.autograd.grad(sum(wi * ri for wi, ri in zip(wr, outs[:4])), rins + [dr], retain_graph=True)
            gy, gy_buf = be.cl(torch.zeros_like(y), extra_rows=2)
            gy.fill_(SENTINEL)
            y_gp = gz = gz_buf = gz_ref = None
            if n_gp:
                z_gp, m_gp = masked_relu_inputs(g, n_gp, nf, H, W, keep)
                zg = z_gp.double().requires_grad_(True)
                D = ((torch.relu(zg) * m_gp.double()).mean(dim=(2, 3)) @ P[0].detach().reshape(-1)).sum()
                (gz_ref,) = torch.autograd.grad(D, zg)
                y_gp = be.cl(torch.relu(z_gp) * m_gp)
                gz, gz_buf = be.cl(torch.zeros_like(z_gp), extra_rows=2)
                gz.fill_(SENTINEL)
            res = K.tail_heads_bwd(be.cl(y), d, f, probs if with_a else None, labd, ct_i, gout, B, lam2, M, scale, ms, Pk[0],
                                   Pk[2] if with_a else None, out=gy, y_gp=y_gp, out_gp=gz)
            assert res[0] is gy
            check_tail_grads('tail_heads bwd', [t for t in res if t is not None], gr[:-1], gr[-1])
            be.sync()
            assert (gy_buf[3 * B:] == SENTINEL).all()
            if n_gp:
                close('gp_head_grad', gz, gz_ref, FWD_TOL)
                assert (gz_buf[n_gp:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ gen_heads_fwd / gen_heads_bwd
# (n, nf, H, W): n > 256 (gen_heads_loss's batch loop), nf > 256 (the t[j] fill's second pass), hw 1 and 49
GEN_HEADS_CASES = [(1, 4, 1, 1), (5, 260, 7, 7), (300, 4, 7, 7), (5, 1024, 7, 7), (300, 260, 1, 1), (1, 1024, 1, 1)]


def check_gen_heads(be, n, nf, H, W, with_a):
    K, F = be.K, be.F
    ncls, keep, go = 10, 0.8, f32(0.6)
    ms, scale = f32(1.0 / keep), f32(0.1)
    g = gen('gh', n, nf, H, W)
    z, mask = masked_relu_inputs(g, n, nf, H, W, keep)
    mask = (mask > 0).float() * ms
    y = torch.relu(z) * mask
    params = list(head_params(g, nf, ncls))
    if not with_a:
        params[2] = params[3] = None
    lab = torch.randint(0, ncls, (n,), generator=g, dtype=torch.int32)
    zr = z.double().requires_grad_(True)
    P = [t.double() if t is not None else None for t in params]
    cost, dr, ar = ref_gen_heads(torch.relu(zr) * mask.double(), *P, lab, scale)
    (gref,) = torch.autograd.grad(cost * go, zr)
    Pd = [be.dev(t) if t is not None else None for t in params]
    yd, labd = be.cl(y), be.dev(lab)
    out, probs, d = K.gen_heads_fwd(yd, *Pd, labd, scale)
    close_scalar('gen_heads fwd', out, cost.detach())
    close('gen_heads fwd d', d, dr.detach(), DOT_TOL)
    assert (probs is None) == (not with_a)
    gy = K.gen_heads_bwd(yd, probs, labd, be.dev(torch.tensor([go])), scale, ms, Pd[0], Pd[2])
    close_l2('gen_heads bwd', gy, gref, float(gref.abs().max()))
    yg = be.cl(y).requires_grad_(True)
    cost2, d2 = F.gen_tail_heads(yg, *Pd, labd, scale, ms)
    close_scalar('gen_heads fwd', cost2, cost.detach())
    assert torch.equal(d2, d)
    (gy2,) = torch.autograd.grad(cost2 * go, yg)
    close_l2('gen_heads bwd', gy2, gref, float(gref.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ gp_head_grad / gp_head_wgrad
# gp_head_wgrad_stage1 cuts the n * hw rows into 64 slices of ceil(rows / 64): rows < 64 leaves most slices empty, 65 gives slices of 2 with the
# last 31 empty, 1000 gives 16 with a ragged last one.  nf / 4 must divide 256: 1, 2, 64, 256 row lanes of 256, 128, 4, 1.
GP_HEAD_ROWS = {1: (1, 1, 1), 63: (7, 3, 3), 64: (4, 4, 4), 65: (5, 1, 13), 1000: (10, 10, 10)}       # rows -> (n, H, W)
GP_HEAD_CASES = [(nf, rows) for nf in (4, 8, 256, 1024) for rows in GP_HEAD_ROWS if (nf, rows) != (1024, 1000)]   # (that one is 4 MB)


def check_gp_head(be, nf, rows):
    K = be.K
    n, H, W = GP_HEAD_ROWS[rows]
    keep = 0.5
    ms = 1.0 / keep
    g = gen('gph', nf, rows)
    z, mask = masked_relu_inputs(g, n, nf, H, W, keep)
    y = torch.relu(z) * mask
    w_out = torch.randn(nf, 1, generator=g)
    gg = torch.randn(n, nf, H, W, generator=g)
    base = torch.randn(nf, 1, generator=g)
    zr = z.double().requires_grad_(True); wr = w_out.double().requires_grad_(True)
    D = ((torch.relu(zr) * mask.double()).mean(dim=(2, 3)) @ wr.reshape(-1)).sum()
    (gz_ref,) = torch.autograd.grad(D, zr, create_graph=True)
    (gw_ref,) = torch.autograd.grad((gz_ref * gg.double()).sum(), wr)           # the adjoint of gz w.r.t. w_out
    yd, wd = be.cl(y), be.dev(w_out)
    close('gp_head_grad', K.gp_head_grad(yd, wd, ms), gz_ref.detach(), FWD_TOL)
    gz, buf = be.cl(torch.zeros_like(y), extra_rows=1)
    assert K.gp_head_grad(yd, wd, ms, out=gz) is gz
    close('gp_head_grad', gz, gz_ref.detach(), FWD_TOL)
    be.sync()
    assert (buf[n:] == SENTINEL).all()
    gw = K.gp_head_wgrad(be.cl(gg), yd, ms, wd)
    assert tuple(gw.shape) == (nf, 1)
    close('gp_head_wgrad', gw, gw_ref, GRAD_TOL)
    acc = be.dev(base)
    assert K.gp_head_wgrad(be.cl(gg), yd, ms, wd, add_to=acc) is acc
    close('gp_head_wgrad', acc, base.double() + gw_ref, GRAD_TOL)


def check_gp_head_grad_large(be):
    """n * hw * nf / 4 past 4096 blocks of 256 threads: gp_head_grad_kernel takes one float4 per thread and has no stride loop, so a capped
    grid leaves the end of gz unwritten - which only a tensor of more than 4,194,304 elements shows (the 64 x 64 critic at batch 129: 16.1 MiB)"""
    n, nf, H, W, keep = 129, 512, 8, 8, 0.5
    assert n * nf * H * W // 4 > 4096 * 256
    g = gen('gph-large')
    z, mask = masked_relu_inputs(g, n, nf, H, W, keep)
    w_out = torch.randn(nf, 1, generator=g)
    zr = z.double().requires_grad_(True)
    D = ((torch.relu(zr) * mask.double()).mean(dim=(2, 3)) @ w_out.double().reshape(-1)).sum()
    (gz_ref,) = torch.autograd.grad(D, zr)
    gz, buf = be.cl(torch.zeros_like(z), extra_rows=1)
    gz.fill_(SENTINEL)
    be.K.gp_head_grad(be.cl(torch.relu(z) * mask), be.dev(w_out), 1.0 / keep, out=gz)
    close('gp_head_grad', gz[-1:], gz_ref[-1:], FWD_TOL)          # the last sample first: the rows a capped grid would miss
    close('gp_head_grad', gz, gz_ref, FWD_TOL)
    be.sync()
    assert (buf[n:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ gp_finish
GP_FINISH_CASES = [(B, C, H, W, lay) for (B, C, H, W) in ((1, 1, 2, 2), (5, 3, 6, 10)) for lay in ('nchw', 'cl', 'slice')]


def check_gp_finish(be, B, C, H, W, layout):
    g = gen('gpf', B, C, H, W)
    ga = torch.randn(B, C, H, W, generator=g)
    big = torch.randn(B, C + 1, H // 2 + 1, W // 2 + 2, generator=g)
    gs = big[:, 1:, :H // 2, 1:1 + W // 2]
    scale = 0.25
    v_ref, s_ref = ref_gp_finish(ga.double(), gs.double(), scale)
    if layout == 'nchw':
        gsd = be.dev(gs)
    elif layout == 'cl':
        gsd = be.cl(gs.contiguous())
    else:
        gsd = be.dev(big)[:, 1:, :H // 2, 1:1 + W // 2]
        assert not gsd.is_contiguous() or gsd.numel() == 1
    gad = be.dev(ga)
    slopes = be.K.gp_finish(gad, gsd, scale)
    close('gp_finish', slopes, s_ref, FWD_TOL)
    close('gp_finish', gad, v_ref, FWD_TOL)
