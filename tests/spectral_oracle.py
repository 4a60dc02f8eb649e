"""fp64 restatement of the spectral normalisation (csrc/spectral.hip, optim.SpectralNorm; Miyato et al., ICLR 2018) and the worst-case
rounding bounds its fp32 kernels are held to.  numpy only; nothing under ctgan_amd/ imports this file.

    t = M u;  v = t / max(|t|, eps);  s = M^T v;  sigma = |s|;  u' = s / max(sigma, eps);  Mbar = M / max(sigma, eps)
    G = (Gbar - <Gbar, Mbar> v u'^T) / max(sigma, eps)

THE BOUNDS.  e = 2^-24 is the unit roundoff of fp32, g(n) = n e / (1 - n e).  An n-term fp32 sum of products (fused or not, in ANY order)
errs by at most g(n) sum|a_i b_i|; a square root, a division or a product adds a relative e.  Below |x| is the Euclidean norm, abs(x) the
elementwise absolute value, everything on the right is evaluated in fp64 from the fp32 inputs, and second-order terms are covered by the
factor SLACK = 1.01 on the whole (n e <= 3e-4 for every shape in the tree).  Absolute error bounds, composed along the chain:

    dt     = g(N) abs(M) abs(u)                                        [K]   the N-term dot of a row
    d|t|   = |dt| + (g(K) / 2 + e) |t|                                       (||t+dt| - |t|| <= |dt|; the K-term sum of squares, the root)
    dv     = dt / |t| + abs(v) (d|t| / |t| + e)                        [K]   the quotient t / |t|
    ds     = abs(M)^T dv + g(K) abs(M)^T abs(v) + abs(s) (d|t| / |t| + e)    [N]
             (the kernel sums M^T t over K terms and divides by its |t| afterwards: first the input error, then the sum's, then the scalar's)
    dsigma = |ds| + (g(N) / 2 + e) sigma
    du     = ds / sigma + abs(u') (dsigma / sigma + e)                 [N]
    dMbar  = abs(Mbar) (dsigma / sigma + e)                            [K, N]
    ddot   = sum(abs(Gbar) dMbar) + g(K N) sum(abs(Gbar) abs(Mbar))          <Gbar, Mbar>, a K N-term dot
    dG     = ( ddot abs(v) abs(u')^T + abs(dot) (dv abs(u')^T + abs(v) du^T) + 3 e abs(dot) abs(v) abs(u')^T + e abs(Gbar - dot v u'^T) ) / sigma
             + abs(G) (dsigma / sigma + e)                             [K, N]

(the bounds need |t| > 0 and sigma > 0; the all-zero matrix is checked for exact zeros instead)."""
import numpy as np

EPS = 1e-12
E32 = 2.0 ** -24
SLACK = 1.01


def gamma(n):
    return n * E32 / (1.0 - n * E32)


def normalise(M, u):
    """-> dict(t, nt, v, s, sigma, u, Mbar), all fp64, from M [K, N] and u [N]"""
    M = np.asarray(M, np.float64); u = np.asarray(u, np.float64)
    t = M @ u
    nt = np.sqrt((t * t).sum())
    v = t / max(nt, EPS)
    s = M.T @ v
    sigma = np.sqrt((s * s).sum())
    return dict(t=t, nt=nt, v=v, s=s, sigma=sigma, u=s / max(sigma, EPS), Mbar=M / max(sigma, EPS))


def grad(Gbar, Mbar, u, v, sigma):
    """G from Gbar = dL/dMbar, with u (the new one), v constants"""
    Gbar = np.asarray(Gbar, np.float64); Mbar = np.asarray(Mbar, np.float64)
    dot = (Gbar * Mbar).sum()
    return (Gbar - dot * np.outer(np.asarray(v, np.float64), np.asarray(u, np.float64))) / max(float(sigma), EPS)


def normalise_bounds(M, u):
    """-> (the fp64 results of normalise, dict of absolute error bounds for v, sigma, u, Mbar) per the module docstring"""
    r = normalise(M, u)
    A = np.abs(np.asarray(M, np.float64)); au = np.abs(np.asarray(u, np.float64))
    K, N = A.shape
    nt, sg = r['nt'], r['sigma']
    dt = gamma(N) * (A @ au)
    dnt = np.sqrt((dt * dt).sum()) + (gamma(K) / 2 + E32) * nt
    dv = dt / nt + np.abs(r['v']) * (dnt / nt + E32)
    ds = A.T @ dv + gamma(K) * (A.T @ np.abs(r['v'])) + np.abs(r['s']) * (dnt / nt + E32)
    dsg = np.sqrt((ds * ds).sum()) + (gamma(N) / 2 + E32) * sg
    du = ds / sg + np.abs(r['u']) * (dsg / sg + E32)
    dMbar = np.abs(r['Mbar']) * (dsg / sg + E32)
    return r, {k: SLACK * x for k, x in dict(v=dv, sigma=dsg, u=du, Mbar=dMbar).items()}


def grad_bound(Gbar, M, u0):
    """-> (fp64 G, its absolute error bound [K, N], the fp64 normalise results): the whole chain u0 -> (u', v, sigma, Mbar) -> G"""
    r, b = normalise_bounds(M, u0)
    Gbar = np.asarray(Gbar, np.float64)
    K, N = Gbar.shape
    sg = r['sigma']
    G = grad(Gbar, r['Mbar'], r['u'], r['v'], sg)
    dot = (Gbar * r['Mbar']).sum()
    av, au = np.abs(r['v']), np.abs(r['u'])
    ddot = (np.abs(Gbar) * b['Mbar']).sum() + gamma(K * N) * (np.abs(Gbar) * np.abs(r['Mbar'])).sum()
    num = (ddot * np.outer(av, au) + abs(dot) * (np.outer(b['v'], au) + np.outer(av, b['u'])) + 3 * E32 * abs(dot) * np.outer(av, au)
           + E32 * np.abs(Gbar - dot * np.outer(r['v'], r['u'])))
    dG = num / sg + np.abs(G) * (b['sigma'] / sg + E32)
    return G, SLACK * dG, r
