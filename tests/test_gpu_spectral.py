"""Spectral normalisation kernels on the MI355X (`-m gpu`; csrc/spectral.hip through kernels.spectral_normalize / spectral_grad) against
the fp64 restatement and the worst-case rounding bounds of tests/spectral_oracle.py.  ONE bucket holds every shape at which the kernels take
another path, separated by unnormalised gaps of 1 and 3 elements so that no offset but the first is 16-byte aligned and several are odd
multiples of 4 bytes.

THE BOUNDS are the closed forms of tests/spectral_oracle.py's docstring (e = 2^-24, g(n) = n e / (1 - n e); K, N the matrix; everything on
the right in fp64):  dt = g(N) abs(M) abs(u);  d|t| = |dt| + (g(K)/2 + e) |t|;  dv = dt/|t| + abs(v) (d|t|/|t| + e);
ds = abs(M)^T dv + g(K) abs(M)^T abs(v) + abs(s) (d|t|/|t| + e);  dsigma = |ds| + (g(N)/2 + e) sigma;  du = ds/sigma + abs(u') (dsigma/sigma + e);
dMbar = abs(Mbar) (dsigma/sigma + e);  ddot = sum(abs(Gbar) dMbar) + g(K N) sum(abs(Gbar) abs(Mbar));
dG = (ddot abs(v) abs(u')^T + abs(dot) (dv abs(u')^T + abs(v) du^T) + 3 e abs(dot) abs(v) abs(u')^T + e abs(Gbar - dot v u'^T)) / sigma
     + abs(G) (dsigma/sigma + e);  all times 1.01 for the second-order terms.  Each test prints its largest observed error / bound ratio."""
import numpy as np
import pytest
import torch

from tests import spectral_oracle as O

pytestmark = pytest.mark.gpu

ZERO = 10                  # index of the all-zero matrix in shapes()


@pytest.fixture(scope='module')
def K():
    import ctgan_amd.kernels as K
    return K


def shapes(K):
    return [(1, 1), (1, 7), (5, 1), (3, 128), (27, 128), (128, 10), (129, 13), (1152, 128), (1153, 64), (2049, 3), (16, 16),
            (8, K.SPECTRAL_MAX_N)]


def _layout(shp):
    """-> (jobs [(offset, K, N)], total): a gap of 1 or 3 unnormalised elements behind every matrix - 1 where that makes the next offset
    odd (an odd multiple of 4 bytes), else whichever keeps it off the 16-byte grid (then it is 2 mod 4: 8-byte aligned at best)"""
    jobs, off = [], 0
    for k, n in shp:
        jobs.append((off, k, n))
        end = off + k * n
        off = end + (1 if (end + 1) % 4 else 3)
    return jobs, off


class Bucket:
    """theta, the state and the table of `shp` on the device; matrices and u drawn per shape from its own seed (the same wherever it sits)"""

    def __init__(self, K, shp, zero=()):
        self.K, self.shp = K, shp
        self.jobs, self.total = _layout(shp)
        theta = torch.randn(self.total, generator=torch.Generator().manual_seed(99)) * 3.0         # (the gaps keep these values)
        us = []
        for i, ((o, k, n), s) in enumerate(zip(self.jobs, shp)):
            g = torch.Generator().manual_seed(1000 * k + n)
            theta[o:o + k * n] = 0.0 if i in zero else torch.randn(k * n, generator=g) * 0.05
            u = torch.randn(n, generator=g)
            us.append(u / u.norm())
        self.theta_h, self.u0_h = theta, torch.cat(us)
        dev = torch.device('cuda')
        self.table = K.SpectralTable(self.jobs, self.total, dev)
        self.theta = theta.to(dev)
        self.bar = torch.full_like(self.theta, float('nan'))
        self.u, self.v = self.u0_h.to(dev), torch.full((self.table.v_size,), float('nan'), device=dev)
        self.sigma = torch.full((len(shp),), float('nan'), device=dev)
        self.scratch = torch.full((self.table.scratch_floats,), float('nan'), device=dev)

    def normalise(self, iterate=True):
        self.K.spectral_normalize(self.theta, self.bar, self.table, self.u, self.v, self.sigma, self.scratch, iterate=iterate)

    def grad(self, g):
        self.K.spectral_grad(g, self.bar, self.table, self.u, self.v, self.sigma, self.scratch)

    def part(self, i, host):
        """(M or Mbar [K, N], u [N], v [K], sigma) of job i from the host copies host = (flat, u, v, sigma)"""
        (o, k, n), uo, vo = self.jobs[i], self.table.u_offs[i], self.table.v_offs[i]
        return host[0][o:o + k * n].view(k, n), host[1][uo:uo + n], host[2][vo:vo + k], host[3][i]

    def host(self):
        return self.bar.cpu(), self.u.cpu(), self.v.cpu(), self.sigma.cpu()

    def gap_mask(self):
        m = torch.ones(self.total, dtype=torch.bool)
        for o, k, n in self.jobs:
            m[o:o + k * n] = False
        return m


@pytest.fixture(scope='module')
def grouped(K):
    """the bucket after ONE normalise from u0 (shared, left unchanged) -> (bucket, host copies)"""
    b = Bucket(K, shapes(K), zero=(ZERO,))
    b.normalise()
    torch.cuda.synchronize()
    return b, b.host()


def test_table_and_launch_counts(K):
    assert K.SPECTRAL_MAX_N >= 1024 and [K.spectral_launches(w) for w in ('normalise', 'rescale', 'grad')] == [3, 1, 2]
    jobs, total = _layout(shapes(K))
    assert all(o % 4 for o, _, _ in jobs[1:]) and sum(o % 2 for o, _, _ in jobs) >= 4       # none 16-byte aligned, several odd
    assert {jobs[i + 1][0] - (o + k * n) for i, (o, k, n) in enumerate(jobs[:-1])} == {1, 3}
    with pytest.raises(NotImplementedError):
        K.SpectralTable([(0, 2, K.SPECTRAL_MAX_N + 1)], 4 * K.SPECTRAL_MAX_N, torch.device('cpu'))
    for bad in ([(0, 4, 4), (8, 4, 4)], [(4, 2, 2), (0, 2, 2)], [(0, 0, 3)]):          # overlaps its neighbour (and leaves the bucket); out of order; empty
        with pytest.raises(ValueError):
            K.SpectralTable(bad, 20, torch.device('cpu'))


def test_normalise_against_fp64_within_the_derived_bound(K, grouped):
    b, host = grouped
    worst = {}
    for i, (k, n) in enumerate(b.shp):
        Mbar, u, v, sg = b.part(i, host)
        M = b.part(i, (b.theta_h, b.u0_h, host[2], host[3]))[0]
        u0 = b.part(i, (b.theta_h, b.u0_h, host[2], host[3]))[1]
        if i == ZERO:
            assert float(sg) == 0.0 and not Mbar.any() and not u.any() and not v.any()            # zeros, and finite
            continue
        r, bound = O.normalise_bounds(M.numpy(), u0.numpy())
        for key, got in (('v', v), ('sigma', sg), ('u', u), ('Mbar', Mbar)):
            err = np.abs(got.numpy().astype(np.float64) - r[key])
            ratio = float(np.max(err / np.maximum(bound[key], 1e-300)))
            worst[key] = max(worst.get(key, 0.0), ratio)
            assert ratio <= 1.0, (b.shp[i], key, ratio)
        # Mbar max(sigma, eps) gives M back to 2 ulp
        back = Mbar * sg.clamp_min(1e-12)
        ulp = torch.nextafter(torch.abs(M), torch.full_like(M, float('inf'))) - torch.abs(M)          # the spacing of fp32 at M
        assert bool((torch.abs(back - M) <= 2 * ulp).all()), b.shp[i]
    print('normalise: largest error / bound', {k: round(x, 4) for k, x in worst.items()})
    gaps = b.gap_mask()
    assert gaps.sum() > 0 and torch.equal(host[0][gaps].view(torch.int32), b.theta_h[gaps].view(torch.int32))       # copied bit for bit
    assert all(bool(torch.isfinite(t).all()) for t in host)


def test_same_bits_alone_at_offset_zero_and_on_a_second_run(K, grouped):
    b, host = grouped
    again = Bucket(K, shapes(K), zero=(ZERO,))
    again.normalise()
    for a, c in zip(again.host(), host):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    for i, s in enumerate(b.shp):
        solo = Bucket(K, [s], zero=(0,) if i == ZERO else ())
        assert solo.jobs[0][0] == 0
        solo.normalise()
        for x, y in zip(solo.part(0, solo.host()), b.part(i, host)):
            assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), s


def test_power_iteration_converges_to_the_largest_singular_value(K):
    k, n = 96, 40
    g = torch.Generator().manual_seed(3)
    qa, _ = torch.linalg.qr(torch.randn(k, n, generator=g, dtype=torch.float64))
    qb, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    sv = 2.0 ** (1 - torch.arange(n, dtype=torch.float64))                   # 2, 1, 0.5, ...
    M = ((qa * sv) @ qb.t()).float()
    b = Bucket(K, [(k, n)])
    b.theta[:k * n].copy_(M.reshape(-1).cuda())
    for _ in range(20):
        b.normalise()
    bar, u, v, sg = b.host()
    # after 20 calls the power-method error is (1/2)^40 times a constant: what is left is the rounding of ONE call from the converged u
    M64 = b.theta.cpu()[:k * n].view(k, n).numpy().astype(np.float64)
    true = float(np.linalg.svd(M64, compute_uv=False)[0])
    _, bound = O.normalise_bounds(M64, np.linalg.svd(M64)[2][0])
    ratio = abs(float(sg[0]) - true) / float(bound['sigma'])
    print('converged sigma %.9g (fp64 %.9g): error / bound %.4f' % (float(sg[0]), true, ratio))
    assert abs(true - 2.0) < 1e-6 and ratio <= 1.0


def test_grad_against_fp64_and_autograd(K, grouped):
    b, host = grouped
    gbar_h = torch.randn(b.total, generator=torch.Generator().manual_seed(17))
    gdev = gbar_h.cuda()
    b.grad(gdev)
    got = gdev.cpu()
    gaps = b.gap_mask()
    assert torch.equal(got[gaps].view(torch.int32), gbar_h[gaps].view(torch.int32))                  # untouched bit for bit
    again = gbar_h.cuda()
    b.grad(again)
    assert torch.equal(again.cpu().view(torch.int32), got.view(torch.int32))
    worst = worst_ad = 0.0
    for i, (k, n) in enumerate(b.shp):
        o = b.jobs[i][0]
        Gbar, G = gbar_h[o:o + k * n].view(k, n), got[o:o + k * n].view(k, n)
        M, u0 = b.part(i, (b.theta_h, b.u0_h, host[2], host[3]))[:2]
        if i == ZERO:
            assert bool(torch.isfinite(G).all())            # sigma = 0: Gbar / eps, finite
            continue
        want, bound, r = O.grad_bound(Gbar.numpy(), M.numpy(), u0.numpy())
        ratio = float(np.max(np.abs(G.numpy().astype(np.float64) - want) / np.maximum(bound, 1e-300)))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (b.shp[i], ratio)
        # torch.autograd on the CPU-double restatement M / (v^T M u), u and v detached
        Md = M.double().clone().requires_grad_(True)
        ud, vd = torch.from_numpy(r['u']), torch.from_numpy(r['v'])
        ((Md / (vd @ Md @ ud)) * Gbar.double()).sum().backward()
        ad = float(np.max(np.abs(G.numpy().astype(np.float64) - Md.grad.numpy()) / np.maximum(bound, 1e-300)))
        worst_ad = max(worst_ad, ad)
        assert ad <= 1.0, (b.shp[i], ad)
    print('grad: largest error / bound %.4f (against autograd %.4f)' % (worst, worst_ad))


def test_rescale_only_leaves_the_state_and_reproduces_theta_bar(K, grouped):
    _, host = grouped
    c = Bucket(K, shapes(K), zero=(ZERO,))
    c.normalise()
    c.bar.fill_(float('nan'))
    c.normalise(iterate=False)
    for a, d in zip(c.host(), host):
        assert torch.equal(a.view(torch.int32), d.view(torch.int32))


def test_a_dropped_update_holds_the_iteration(K, grouped):
    """Under a dynamic loss scale: spectral_grad copies the scaler's flag into `hold`, and the normalise that is given `hold` skips the
    iteration on the device when it is set - u, v, sigma and theta_bar keep their bits - and iterates as without it when it is clear."""
    _, host = grouped
    for found in (1.0, 0.0):
        c = Bucket(K, shapes(K), zero=(ZERO,))
        c.normalise()
        scaler = torch.tensor([1024.0, found, 3.0, 0.0], device='cuda')
        hold = torch.full((1,), 7.0, device='cuda')
        g = torch.randn(c.total, generator=torch.Generator().manual_seed(17)).cuda()
        plain = g.clone()
        c.grad(plain)
        K.spectral_grad(g, c.bar, c.table, c.u, c.v, c.sigma, c.scratch, scaler=scaler, hold=hold)
        assert torch.equal(g.view(torch.int32), plain.view(torch.int32)) and float(hold[0]) == found        # the transform itself is the same
        assert scaler.tolist() == [1024.0, found, 3.0, 0.0]
        c.bar.fill_(float('nan'))
        K.spectral_normalize(c.theta, c.bar, c.table, c.u, c.v, c.sigma, c.scratch, hold=hold)
        d = Bucket(K, shapes(K), zero=(ZERO,))
        d.normalise()
        if not found:
            d.normalise()                                          # a second iteration: what the un-held call is
        for a, b in zip(c.host(), d.host()):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), found
        assert (not found) or all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(c.host(), host))
    with pytest.raises(ValueError):
        K.spectral_grad(g, c.bar, c.table, c.u, c.v, c.sigma, c.scratch, scaler=scaler)                  # one without the other
