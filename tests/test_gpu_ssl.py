"""The semi-supervised CT classifier on the MI355X (`-m gpu`): every kernel of csrc/ssl.hip against fp64, one classifier and one
generator step at the script's full sizes against the oracle (tests/ssl_oracle.py) on shared Philox streams, graph replay against
eager and a resumed run against an uninterrupted one bit for bit, a short loop on synthetic ten-class data against the oracle's, and
the product pinned to tests/golden/ssl_step.npz.  Kernel bounds are those of tests/test_gpu_kernels.py for the linear and elementwise
families: max |error| / max |reference| below 2e-5 for forward results and 3e-5 for gradients."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import philox  # noqa: E402
from tests import ssl_oracle as O  # noqa: E402

FWD_TOL, GRAD_TOL = 2e-5, 3e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssl_step.npz')


@pytest.fixture
def K():
    import ctgan_amd.kernels as K
    return K


@pytest.fixture
def clean():
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    yield M
    M.configure(); lib.delete_all_params(); lib.delete_param_aliases()


def dev(t):
    return t.to('cuda')


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    e = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    print('relerr %.3g' % e)
    return e


SHAPES = [(784, 1000), (250, 10), (7, 3), (784, 10), (250, 1000), (7, 1000)]


@pytest.mark.parametrize('n_in,n_out', SHAPES)
@pytest.mark.parametrize('eps', [0.0, 1e-6])
def test_weight_norm_fwd_bwd(K, n_in, n_out, eps):
    g = torch.Generator().manual_seed(n_in + n_out)
    theta = torch.randn(n_in, n_out, generator=g) * 0.1
    s = torch.rand(n_out, generator=g) + 0.5
    gW = torch.randn(n_in, n_out, generator=g)
    w, rnorm = K.wn_fwd(dev(theta), dev(s), eps)
    ref = O.wn_weight(theta.double(), s.double(), eps)
    assert relerr(w, ref) < FWD_TOL
    assert relerr(rnorm, 1.0 / torch.sqrt(eps + (theta.double() ** 2).sum(0))) < FWD_TOL
    gt, gs = K.wn_bwd(dev(gW), dev(theta), dev(s), rnorm)
    ft, fs = O.wn_grad_formula(gW.double(), theta.double(), s.double(), eps)
    assert relerr(gt, ft) < GRAD_TOL and relerr(gs, fs) < GRAD_TOL
    gt2, none = K.wn_bwd(dev(gW), dev(theta), dev(s), rnorm, want_gs=False)
    assert none is None and torch.equal(gt2, gt)


@pytest.mark.parametrize('rows,cols,row_offset', [(401, 1000, 0), (37, 10, 0), (37, 10, 5), (13, 3, 7), (100, 784, 300), (5, 7, 1)])
def test_dense_epilogue_draws_the_documented_stream(K, rows, cols, row_offset):
    # the second stream is corner B of tests/philox_spec.py: high key word, rank bits of the stream id and counter word 3 all non-zero
    for seed, sid, step in ((1234567891011, 6, 3), (0x9E3779B97F4A7C15, (513 << 16) | 7, (1 << 32) + 5)):
        _dense_epilogue_on_stream(K, rows, cols, row_offset, seed, sid, step)


def _dense_epilogue_on_stream(K, rows, cols, row_offset, seed, sid, step):
    sigma = 0.5
    g = torch.Generator().manual_seed(rows + cols)
    y = torch.randn(rows, cols, generator=g)
    b = torch.randn(cols, generator=g)
    ctr = torch.tensor([step], dtype=torch.int64, device='cuda')
    z = philox.normal(seed, sid, step, (row_offset + rows) * cols)[row_offset * cols:].reshape(rows, cols)
    z = torch.from_numpy(z.copy()).double()
    a_ref = torch.relu(y.double() + b.double())
    h, a = K.dense_noise_fwd(dev(y), dev(b), True, sigma, seed, sid, ctr, row_offset, want_a=True)
    assert relerr(a, a_ref) < FWD_TOL and relerr(h, a_ref + sigma * z) < FWD_TOL
    # the input site: no bias, no ReLU; the noise alone equals oracle.philox.normal
    h0, none = K.dense_noise_fwd(dev(y), None, False, 0.3, seed, sid, ctr, row_offset)
    assert none is None and relerr(h0, y.double() + 0.3 * z) < FWD_TOL
    hz, _ = K.dense_noise_fwd(torch.zeros(rows, cols, device='cuda'), None, False, 1.0, seed, sid, ctr, row_offset)
    assert relerr(hz, z) < FWD_TOL
    # a row block of a larger tensor draws what the whole tensor's launch draws there
    if row_offset:
        whole, _ = K.dense_noise_fwd(torch.zeros(row_offset + rows, cols, device='cuda'), None, False, 1.0, seed, sid, ctr, 0)
        assert torch.equal(whole[row_offset:], hz)
    # deterministic: sigma 0 is the activation itself
    hd, _ = K.dense_noise_fwd(dev(y), dev(b), True, 0.0, seed, sid, ctr, row_offset)
    assert torch.equal(hd, a)
    # backward: ReLU mask from the sign of y + b on the summed cotangents, bias gradient in the same launch
    gh, ga = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    mask = (y.double() + b.double() > 0).double()
    gz, gb = K.dense_noise_bwd(dev(gh), dev(ga), dev(y), dev(b), True)
    ref = (gh.double() + ga.double()) * mask
    assert relerr(gz, ref) < GRAD_TOL
    assert (gb.cpu().double() - ref.sum(0)).abs().max().item() < GRAD_TOL * ref.abs().sum(0).max().item()
    gz1, gb1 = K.dense_noise_bwd(dev(gh), None, dev(y), dev(b), True, want_gb=False)
    assert gb1 is None and relerr(gz1, gh.double() * mask) < GRAD_TOL
    gz2, _ = K.dense_noise_bwd(None, dev(ga), dev(y), dev(b), True)
    assert relerr(gz2, ga.double() * mask) < GRAD_TOL


def test_dense_epilogue_autograd(K):
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(0)
    y = dev(torch.randn(33, 10, generator=g)).requires_grad_(True)
    b = dev(torch.randn(10, generator=g)).requires_grad_(True)
    ctr = torch.zeros(1, dtype=torch.int64, device='cuda')
    h, a = F.dense_noise(y, b, True, 0.5, (7, 2, ctr), 0, want_a=True)
    gh = dev(torch.randn(33, 10, generator=g))
    gy, gb = torch.autograd.grad([h, a], [y, b], [gh, gh])
    mask = (y.detach() + b.detach() > 0).double().cpu()
    assert relerr(gy, 2 * gh.cpu().double() * mask) < GRAD_TOL
    x = dev(torch.randn(33, 10, generator=g)).requires_grad_(True)
    (gx,) = torch.autograd.grad(F.dense_noise(x, None, False, 0.3, (7, 3, ctr)), x, gh)
    assert torch.equal(gx, gh)


@pytest.mark.parametrize('rows,cols,relu', [(500, 1000, True), (500, 10, False), (37, 3, True), (9, 250, True)])
def test_init_statistics(K, rows, cols, relu):
    g = torch.Generator().manual_seed(rows + cols)
    y = torch.randn(rows, cols, generator=g) * 3 + torch.randn(cols, generator=g)[None, :]
    s, b = torch.rand(cols, generator=g) + 0.5, torch.zeros(cols)
    yd, sd, bd = dev(y), dev(s), dev(b)
    K.wn_init(yd, sd, bd, relu)
    y64 = y.double()
    mean = y64.mean(0)
    stdv = torch.sqrt(((y64 - mean) ** 2).mean(0))
    ref = (y64 - mean) / stdv
    assert relerr(yd, torch.relu(ref) if relu else ref) < FWD_TOL
    assert relerr(sd, s.double() / stdv) < FWD_TOL and relerr(bd, -mean / stdv) < FWD_TOL


def _head_inputs(B, nc, kind, g):
    if kind == 'random':
        logits = torch.randn(4 * B, nc, generator=g) * 3
    else:                  # +-80 with a few moderate entries, so that both softmaxes have mass on more than one class somewhere
        logits = torch.where(torch.rand(4 * B, nc, generator=g) < 0.5, -80.0, 80.0)
        logits[::3] += torch.randn(logits[::3].shape, generator=g)
    return logits, torch.randint(0, nc, (B,), generator=g, dtype=torch.int32)


@pytest.mark.parametrize('kind', ['random', 'pm80'])
@pytest.mark.parametrize('B,nc', [(100, 10), (37, 10), (300, 10), (5, 3)])
def test_loss_head_fwd_bwd(K, B, nc, kind):
    g = torch.Generator().manual_seed(B + nc)
    logits, labels = _head_inputs(B, nc, kind, g)
    lam2, M = (0.1, 0.0) if B != 37 else (0.1, 0.004)
    out4, ct_i = K.ssl_head_fwd(dev(logits), dev(labels), B, lam2, M)
    x = logits.double().requires_grad_(True)
    ref4, ref_ct = O._head_terms(x, labels, B, lam2, M)
    assert torch.isfinite(out4).all()
    for k in range(4):
        a, b = out4[k].item(), ref4[k].item()
        print(kind, B, nc, k, a, b)
        assert abs(a - b) <= FWD_TOL * max(1.0, abs(b)), (k, a, b)
    assert (ct_i.cpu().double() - ref_ct).abs().max().item() <= FWD_TOL * max(ref_ct.abs().max().item(), 1e-3)
    for gout in ([1.0, 1.0, 0.0, 0.0], [0.3, -2.0, 0.0, 0.0]):
        (gref,) = torch.autograd.grad(ref4[0] * gout[0] + ref4[1] * gout[1], x, retain_graph=True)
        gl = K.ssl_head_bwd(dev(logits), dev(labels), dev(torch.tensor(gout)), B, lam2, M)
        assert torch.isfinite(gl).all() and relerr(gl, gref) < GRAD_TOL


@pytest.mark.parametrize('B,C', [(100, 250), (7, 3), (33, 1000), (100, 10)])
def test_feature_matching_fwd_bwd(K, B, C):
    g = torch.Generator().manual_seed(B + C)
    f = torch.relu(torch.randn(2 * B, C, generator=g) + 0.3)
    x = f.double().requires_grad_(True)
    ref = ((x[:B].mean(0) - x[B:].mean(0)) ** 2).mean()
    loss, diff = K.featmatch_fwd(dev(f), B)
    assert abs(loss.item() - ref.item()) <= FWD_TOL * max(ref.item(), 1e-6)
    (gref,) = torch.autograd.grad(ref, x)
    gf = K.featmatch_bwd(diff, dev(torch.tensor(1.7)), B)
    assert relerr(gf, 1.7 * gref) < GRAD_TOL


@pytest.mark.parametrize('B,C,act', [(100, 500, True), (5, 7, True), (100, 500, False), (33, 3, True)])
def test_batch_norm_2d_softplus_fwd_bwd(K, B, C, act):
    g = torch.Generator().manual_seed(B + C)
    x = torch.randn(B, C, generator=g) * 2 + 1
    off = torch.randn(C, generator=g)
    gy = torch.randn(B, C, generator=g)
    x64, o64 = x.double().requires_grad_(True), off.double().requires_grad_(True)
    c = x64 - x64.mean(0, keepdim=True)
    t = c / torch.sqrt(1e-6 + (c * c).mean(0, keepdim=True)) + o64
    ref = O.softplus(t) if act else t
    y, xhat, rstd = K.bn2d_fwd(dev(x), dev(off), 1e-6, act)
    assert relerr(y, ref) < FWD_TOL
    gx_ref, go_ref = torch.autograd.grad(ref, [x64, o64], gy.double())
    gx, go = K.bn2d_bwd(dev(gy), xhat, dev(off), rstd, act)
    assert relerr(gx, gx_ref) < GRAD_TOL and relerr(go, go_ref) < GRAD_TOL


def test_theano_adam_with_average(K):
    g = torch.Generator().manual_seed(3)
    n = 100003
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * torch.logspace(-6, 1, n)
    m, v, avg = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01, torch.randn(n, generator=g)
    t = 7
    state = dev(torch.tensor([0.003, 0.5 ** t, 0.999 ** t, 0.0]))
    pd, md, vd, ad = dev(p), dev(m), dev(v), dev(avg)
    K.adam_theano_step(pd, dev(gr), md, vd, ad, state, 0.5, 0.999, 1e-8, 1e-4)
    p2, m2, v2 = O.adam_theano(p.double(), gr.double(), m.double(), v.double(), t, 0.003)
    assert relerr(md, m2) < FWD_TOL and relerr(vd, v2) < FWD_TOL
    # the update and the average's move themselves, each within the bound plus the fp32 rounding of the value it is added to
    upd, inc = p2 - p.double(), 1e-4 * (p2 - avg.double())
    e = ((pd.cpu().double() - p.double()) - upd).abs().max().item()
    assert e <= FWD_TOL * upd.abs().max().item() + 2.0 ** -23 * p.abs().max().item(), e
    e = ((ad.cpu().double() - avg.double()) - inc).abs().max().item()
    assert e <= FWD_TOL * inc.abs().max().item() + 2.0 ** -23 * avg.abs().max().item(), e
    # first step from zero slots and zero weights: -lr g / sqrt(g^2 + 1e-8); no average kept
    state = dev(torch.tensor([0.003, 0.5, 0.999, 0.0]))
    pd, md, vd = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    K.adam_theano_step(pd, dev(gr), md, vd, None, state, 0.5, 0.999)
    assert relerr(pd, -0.003 * gr.double() / torch.sqrt(gr.double() ** 2 + 1e-8)) < FWD_TOL
    # non-finite gradients are skipped and counted
    gr2 = gr.clone(); gr2[5] = float('nan'); gr2[77] = float('inf')
    before = pd.clone()
    K.adam_theano_step(pd, dev(gr2), md, vd, None, state, 0.5, 0.999)
    assert state[3].item() == 2 and pd[5] == before[5] and pd[77] == before[77] and torch.isfinite(pd).all()


@pytest.mark.parametrize('n,cin,cout', [(400, 784, 1000), (400, 250, 10), (200, 1000, 500), (37, 7, 3), (400, 250, 250), (100, 100, 500)])
def test_linear_path_at_the_classifier_shapes(K, n, cin, cout):
    """The GEMMs go through functional.linear (the 1x1-conv route): ragged K of 784 / 250, a 10-column output."""
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(n + cin + cout)
    x, w = torch.randn(n, cin, generator=g), torch.randn(cin, cout, generator=g) / np.sqrt(cin)
    gy = torch.randn(n, cout, generator=g)
    xd, wd = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
    y = F.linear(xd, wd)
    print('fwd kernel', K.last_kernel())
    assert relerr(y, x.double() @ w.double()) < FWD_TOL
    gx, gw = torch.autograd.grad(y, [xd, wd], dev(gy))
    assert relerr(gx, gy.double() @ w.double().T) < GRAD_TOL and relerr(gw, x.double().T @ gy.double()) < GRAD_TOL


# ----------------------------------------------------------------------------------------------------- steps, graphs, loop
def test_full_size_steps_match_oracle(clean):
    """Init, one classifier step and one generator step at the script's sizes (B 100, 784-1000-500-250-250-250-10), teacher-forced on
    shared streams: scalars and ct_i within 2e-4, gradients within relative L2 max(3e-3, 3 x fp32 twin), updates and averages by the
    update_ok rule."""
    clean.configure()
    assert O.run_steps('cuda', cost_tol=2e-4, grad_tol=3e-3, log=print) == 13 + 7


def test_product_is_pinned_to_the_committed_fixture(clean):
    """The reduced-width steps against the oracle, whose outputs in the same run equal tests/golden/ssl_step.npz."""
    O.small_cfg()
    got = {}
    assert O.run_steps('cuda', cost_tol=2e-4, grad_tol=3e-3, golden=got) == 13 + 7
    assert O.golden_matches(got, np.load(GOLDEN)) > 30


def _state(tr):
    import ctgan_amd.tflib as lib
    return ([p.detach().clone() for p in lib._params.values()], [t.clone() for o in (tr.d_opt, tr.g_opt) for t in o.slots()],
            int(tr.rng.ctr.item()), tr.d_opt.t, tr.g_opt.t)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and a[2:] == b[2:]


def test_graph_replay_and_resume_are_bit_exact(clean, tmp_path):
    """Six iterations at the script's sizes: graph replay == eager (parameters, averages, Adam slots, counters) and, from a checkpoint
    after three, a resumed graphed run == the uninterrupted one."""
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.engine import GraphedSSLTrainer
    M = clean
    cfg = M.configure()
    g = torch.Generator().manual_seed(4)
    B = cfg.BATCH_SIZE
    batches = [(torch.rand(B, cfg.IN_DIM, generator=g), torch.randint(0, 10, (B,), generator=g, dtype=torch.int32),
                torch.rand(B, cfg.IN_DIM, generator=g), torch.rand(B, cfg.IN_DIM, generator=g)) for _ in range(6)]
    x0 = torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=g)
    P = O.make_params(cfg, seed=8, dtype=torch.float32)

    def fresh():
        lib.delete_all_params()
        tr = M.SSLTrainer(seed=21)
        O.load_into_registry(P)
        return tr
    tr = fresh()
    tr.init_params(dev(x0))
    outs_e = []
    for b in batches:
        outs_e.append(tr.train_iteration(*[dev(t) for t in b])['out4'].clone())
    eager = _state(tr)
    assert tr.d_opt.skipped() == 0 and all(torch.isfinite(o).all() for o in outs_e)

    tr = fresh()
    tr.init_params(dev(x0))
    eng = GraphedSSLTrainer(tr)
    assert eng.graphed, eng.graph_error
    path = str(tmp_path / 'ck.pt')
    for i, b in enumerate(batches):
        out = eng.train_iteration(*b)
        assert torch.equal(out['out4'], outs_e[i]), i
        if i == 2:
            checkpoint.save(path, tr, 3)
    assert _same(_state(tr), eager)

    tr = fresh()
    assert checkpoint.load(path, tr) == 3
    eng = GraphedSSLTrainer(tr)
    assert eng.graphed, eng.graph_error
    for b in batches[3:]:
        eng.train_iteration(*b)
    assert _same(_state(tr), eager)


def test_short_loop_on_synthetic_data_tracks_the_oracle(clean):
    """150 iterations at reduced widths (ssl_oracle.LOOP_CFG) on ten class prototypes + N(0, 0.15^2) noise, 10 labelled examples per
    class, 400 training and 200 test examples.  Chosen on the CPU from the oracle alone: the fp64 oracle reaches a LIVE-weight test
    error of 0.005 (1 of 200; chance is 0.9) - the averaged weights, moved by 1e-4 per step from zero, are still near zero after 150
    steps (oracle: 0.63), so the live weights are compared.  fp32 trajectories leave the fp64 one after tens of steps, so the product
    need not misclassify the same examples: margin 0.025 = five test examples."""
    M = clean
    cfg = M.configure(**O.LOOP_CFG)
    data = O.synthetic_data(cfg, spread=0.15)
    batches = O.loop_batches(cfg, data, 150)
    ref_live, ref_avg = O.loop_oracle(cfg, data, batches)
    live, avg = O.loop_product(cfg, data, batches, 'cuda', graphed=True)
    print('oracle live %.4f avg %.4f; product live %.4f avg %.4f' % (ref_live, ref_avg, live, avg))
    assert ref_live <= 0.01
    assert abs(live - ref_live) <= 0.025, (live, ref_live)


def test_train_runs_graphed_from_an_npz_file(clean, tmp_path):
    M = clean
    M.configure(HIDDEN=(64, 32, 16, 16, 16), G_HIDDEN=(32, 32), BATCH_SIZE=20, COUNT=2, INIT_ROWS=50)
    r = np.random.RandomState(0)
    mk = lambda n: (r.rand(n, 784).astype(np.float32), (np.arange(n) % 10).astype(np.int64))      # noqa: E731
    (xt, yt), (xv, yv), (xs, ys) = mk(80), mk(20), mk(40)
    path = str(tmp_path / 'mnist.npz')
    np.savez(path, x_train=xt, y_train=yt, x_valid=xv, y_valid=yv, x_test=xs, y_test=ys)
    lines = []
    tr = M.train(path, epochs=2, out_dir=str(tmp_path), log=lines.append)
    assert len(lines) == 2 and lines[1].startswith('Iteration 1, time = ') and 'test err = ' in lines[1]
    assert tr.iteration == 10 and tr.d_opt.t == 10 and tr.d_opt.skipped() == 0
