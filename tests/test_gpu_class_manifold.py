"""Per-class precision, recall and kernel distance of conditional samples on the MI355X (`-m gpu`): the grouped kernels of csrc/knn.hip
(ctgan_knn_radii_seg, ctgan_knn_cover_seg) and csrc/kid.hip (ctgan_kernel_tile_sums_seg, ctgan_segment_sums), and
ctgan_amd.score_cifar's labelled FeatureSet / class_precision_recall / class_kernel_distance / class references end to end.

Two kinds of check.  (1) The contract: every class of a grouped launch holds the BITS the pooled entry point leaves from the gathered
rows of that class - no tolerance.  (2) The fp64 oracle applied class by class (tests/class_manifold_oracle.py), with the bounds of
tests/knn_oracle.py and tests/kid_oracle.py and no other: distances and radii within the bound of their own pair, exactly 0 between
bit-identical rows; coverage equal on every row the oracle can decide (on these inputs: every row, tests/test_class_manifold_host.py;
the tests still state the condition and the cap); the nearest index equal where it is unambiguous; kid within e_kid.  The largest
error / bound ratios go to class_manifold_err.json in the run-output directory.

Named to be collected after tests/test_gpu_kernels.py, as tests/test_gpu_score_cifar_frechet.py explains."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import class_manifold_oracle as CO  # noqa: E402
from tests import eval_helpers as H  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402
from tests.test_gpu_score_cifar import K, _full_width_trainer, clean  # noqa: E402,F401  (fixtures and helpers)

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
POOLED_KEYS = ('precision', 'recall', 'nn_dist', 'nn_zero', 'kid', 'kid_std', 'kid_blocks')
CLASS_KEYS = ('precision_class', 'recall_class', 'nn_dist_class', 'nn_zero_class', 'n_class', 'n_class_reference', 'intra_precision',
              'intra_recall', 'kid_class', 'intra_kid')
UNDECIDABLE_CAP = 0.01
# (case, which operands are sliced 4 bytes off a 16-byte boundary): d = 17 has no float4 path either way; at d = 16 the alignment alone decides
LAYOUTS = [(name, ()) for name in CO.NAMES] + [('L4', ('a', 'b')), ('L5', ('b',)), ('L5', ('a',))]
_RATIOS = {}


def _report(key, ratio):
    _RATIOS[key] = max(float(ratio), _RATIOS.get(key, 0.0))
    with open(os.path.join(O.report_dir(), 'class_manifold_err.json'), 'w') as f:
        json.dump({'largest_error_over_bound': _RATIOS}, f, indent=1, sort_keys=True)


def _ratio(err, bound):
    """max err / bound over the elements (an element with a zero bound must have a zero error)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _sentinel(rows, dtype, value, tail=5):
    return torch.full((rows + tail,), value, dtype=dtype, device='cuda')


def _off_by_4_bytes(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


class _Series:
    def __init__(self):
        self.rows = []

    def add(self, name, value):
        self.rows.append((name, value))


class _Sorted:
    """A case's two operands on the device, class-sorted by kernels.class_segments, with the gathered rows of every class."""

    def __init__(self, K, c, unaligned=()):
        self.la, self.lb = torch.from_numpy(c.la).cuda(), torch.from_numpy(c.lb).cuda()
        a, b = torch.from_numpy(c.a).cuda(), torch.from_numpy(c.b).cuda()
        (pa, self.sa), (pb, self.sb) = K.class_segments(self.la, c.classes), K.class_segments(self.lb, c.classes)
        self.fa, self.fb = a.index_select(0, pa).contiguous(), b.index_select(0, pb).contiguous()
        if 'a' in unaligned:
            self.fa = _off_by_4_bytes(self.fa)
        if 'b' in unaligned:
            self.fb = _off_by_4_bytes(self.fb)
        self.ga = [a[self.la == i].contiguous() for i in range(c.classes)]
        self.gb = [b[self.lb == i].contiguous() for i in range(c.classes)]
        self.ha, self.hb = self.sa.tolist(), self.sb.tolist()          # (the TEST reads the counts on the host; the wrappers never do)
        self.m, self.n = self.fa.shape[0], self.fb.shape[0]


# ----------------------------------------------------------------------------------------------------- the contract: the pooled bits
@pytest.mark.parametrize('name,unaligned', LAYOUTS)
def test_every_class_holds_the_bits_of_the_pooled_kernels_on_its_gathered_rows(K, name, unaligned):
    c = CO.case(name)
    s, k, inf = _Sorted(K, c, unaligned), c.k, float('inf')
    # radii of either set
    radii = {}
    for key, f, seg, h, g, rows in (('a', s.fa, s.sa, s.ha, s.ga, s.m), ('b', s.fb, s.sb, s.hb, s.gb, s.n)):
        out = _sentinel(rows, torch.float64, -7.0)
        assert K.knn_radii_seg(f, seg, k, out=out) is out
        assert (out[h[-1]:] == -7.0).all().item()                               # rows of no class and the tail: not written
        for i in range(c.classes):
            got = out[h[i]:h[i + 1]]
            if g[i].shape[0] >= k + 1:
                assert torch.equal(got, K.knn_radii(g[i], k)), (key, i)
            else:
                assert (got == inf).all().item(), (key, i)                      # the selection never fills
        assert torch.equal(K.knn_radii_seg(f, seg, k)[:h[-1]], out[:h[-1]])    # a second run: the same bits
        radii[key] = out[:rows].contiguous()
    # coverage and nearest neighbours, both directions
    for key, (f, seg, h, g, rows), (fo, sego, ho, go, _), r2 in (
            ('ab', (s.fa, s.sa, s.ha, s.ga, s.m), (s.fb, s.sb, s.hb, s.gb, s.n), radii['b']),
            ('ba', (s.fb, s.sb, s.hb, s.gb, s.n), (s.fa, s.sa, s.ha, s.ga, s.m), radii['a'])):
        r2 = r2.clone()
        r2[ho[-1]:] = 0.0                                                        # (what lies behind the last class is never read)
        bufs = _sentinel(rows, torch.int32, -3), _sentinel(rows, torch.float64, -7.0), _sentinel(rows, torch.int32, -5)
        got = K.knn_cover_seg(f, seg, fo, sego, r2, *bufs)
        assert all(x is y for x, y in zip(got, bufs))
        assert (bufs[0][h[-1]:] == -3).all().item() and (bufs[1][h[-1]:] == -7.0).all().item() and (bufs[2][h[-1]:] == -5).all().item()
        for i in range(c.classes):
            cov, d2, idx = (t[h[i]:h[i + 1]] for t in bufs)
            if go[i].shape[0] == 0:                                               # a class with no rows on the other side
                assert (cov == 0).all().item() and (d2 == inf).all().item() and (idx == -1).all().item(), (key, i)
            elif g[i].shape[0]:
                want = K.knn_cover(g[i], go[i], r2[ho[i]:ho[i + 1]].contiguous())
                assert torch.equal(cov, want[0]) and torch.equal(d2, want[1]) and torch.equal(idx, want[2]), (key, i)
        again = K.knn_cover_seg(f, seg, fo, sego, r2)
        assert all(torch.equal(x[:h[-1]], y[:h[-1]]) for x, y in zip(again, bufs))
        none, d2_only, idx_only = K.knn_cover_seg(f, seg, fo, sego)
        assert none is None and torch.equal(d2_only[:h[-1]], bufs[1][:h[-1]]) and torch.equal(idx_only[:h[-1]], bufs[2][:h[-1]])
    # the tile sums: across, and either set against itself without its diagonal
    for key, (f, seg, h, g), (fo, sego, ho, go), diag in (('xy', (s.fa, s.sa, s.ha, s.ga), (s.fb, s.sb, s.hb, s.gb), False),
                                                         ('xx', (s.fa, s.sa, s.ha, s.ga), (s.fa, s.sa, s.ha, s.ga), True),
                                                         ('yy', (s.fb, s.sb, s.hb, s.gb), (s.fb, s.sb, s.hb, s.gb), True)):
        sums, toff = K.kernel_tile_sums_seg(f, seg, fo, sego, exclude_diag=diag)
        t = toff.tolist()
        tiles = lambda rows: -(-rows // K.KERNEL_TILE)          # noqa: E731
        assert toff.dtype == torch.int64 and t[0] == 0
        assert sums.numel() == (tiles(f.shape[0]) + c.classes) * (tiles(fo.shape[0]) + 1) >= t[-1]
        for i in range(c.classes):
            assert t[i + 1] - t[i] == tiles(g[i].shape[0]) * tiles(go[i].shape[0])
            if t[i + 1] > t[i]:
                assert torch.equal(sums[t[i]:t[i + 1]], K.kernel_tile_sums(g[i], go[i], exclude_diag=diag).reshape(-1)), (key, i)
        assert (sums[t[-1]:] == 0).all().item()                                   # what no class owns stays as the wrapper zeroed it
        buf = torch.full_like(sums, -7.0)
        again, toff2 = K.kernel_tile_sums_seg(f, seg, fo, sego, exclude_diag=diag, out=buf)
        assert again is buf and torch.equal(again, sums) and torch.equal(toff2, toff)          # a second run: the same bits
        totals = K.segment_sums(sums, toff)
        for i in range(c.classes):                                                # one fixed order: within the any-order bound of fsum
            v = sums[t[i]:t[i + 1]].tolist()
            assert abs(totals[i].item() - math.fsum(v)) <= max(len(v) - 1, 0) * 2.0 ** -53 * math.fsum(abs(x) for x in v), (key, i)


# ----------------------------------------------------------------------------------------------------- the oracle, class by class
@pytest.mark.parametrize('name', CO.NAMES)
def test_grouped_kernels_match_the_oracle_class_by_class(K, name):
    c = CO.case(name)
    s, k = _Sorted(K, c), c.k
    r2b, r2a = K.knn_radii_seg(s.fb, s.sb, k).cpu().numpy(), K.knn_radii_seg(s.fa, s.sa, k).cpu().numpy()
    cov, d2, idx = (t.cpu().numpy() for t in K.knn_cover_seg(s.fa, s.sa, s.fb, s.sb, torch.from_numpy(r2b).cuda()))
    back = K.knn_cover_seg(s.fb, s.sb, s.fa, s.sa, torch.from_numpy(r2a).cuda())[0].cpu().numpy()
    left, rows = CO.undecidable(c.of)
    assert left <= UNDECIDABLE_CAP * rows
    q_r = q_d = 0.0
    for i, o in enumerate(c.of):
        ra, rb = slice(s.ha[i], s.ha[i + 1]), slice(s.hb[i], s.hb[i + 1])
        if o.r2_b is not None:
            q_r = max(q_r, _ratio(np.abs(r2b[rb] - o.r2_b), o.e_r2_b))
        if o.r2_a is not None:
            q_r = max(q_r, _ratio(np.abs(r2a[ra] - o.r2_a), o.e_r2_a))
        if o.nn_d2 is None:
            continue
        q_d = max(q_d, _ratio(np.abs(d2[ra] - o.nn_d2), o.e_nn))                  # (a zero bound - bit-identical rows - asks for the exact 0)
        assert ((idx[ra] >= 0) & (idx[ra] < o.n)).all() and np.array_equal(idx[ra][o.nn_sure], o.nn_idx[o.nn_sure]), i
        if o.covered is not None:
            assert np.array_equal(cov[ra][o.decidable].astype(bool), o.covered[o.decidable]), i
        if o.back is not None:
            assert np.array_equal(back[rb][o.back_decidable].astype(bool), o.back[o.back_decidable]), i
    zeros = sum(int((o.nn_d2 == 0).sum()) for o in c.of if o.nn_d2 is not None)
    print('%s: |r2 - ref| / bound %.3e, |nn_d2 - ref| / bound %.3e, %d of %d rows undecidable, %d distances exactly 0' % (name, q_r, q_d, left, rows, zeros))
    _report('radii_%s' % name, q_r)
    _report('nearest_%s' % name, q_d)
    assert q_r <= 1.0 and q_d <= 1.0
    assert int((d2[:s.ha[-1]] == 0).sum()) == zeros
    if name == 'L5_planted':                                                      # copies inside one class: exact zeros, radii of exactly 0
        assert zeros == 6 and (r2b[10:11 + k] == 0).all() and (r2b == 0).sum() == k + 1 and idx[CO.KO.COPY_OF_B10] == 10
        assert (cov[[0, 1, 2, 3, 4, CO.KO.COPY_OF_B10]] == 1).all()
    # through score_cifar: the dicts of the two functions
    from ctgan_amd.score_cifar import FeatureSet, class_kernel_distance, class_precision_recall
    fa, fb = FeatureSet(c.a, labels=c.la, classes=c.classes), FeatureSet(c.b, labels=c.lb, classes=c.classes)
    got, want = class_precision_recall(fa, fb, k=k), c.result
    for key in ('n_class', 'n_class_reference', 'nn_zero_class'):
        assert np.array_equal(got[key], want[key]), key
    for key, n_key, flags in (('precision_class', 'n_class', 'decidable'), ('recall_class', 'n_class_reference', 'back_decidable')):
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
        for i, o in enumerate(c.of):
            if not np.isnan(want[key][i]):                                        # the counts differ by at most the class's undecidable rows
                assert abs(got[key][i] - want[key][i]) * want[n_key][i] <= (~getattr(o, flags)).sum() + 1e-9, (key, i)
    assert np.array_equal(np.isnan(got['nn_dist_class']), np.isnan(want['nn_dist_class']))
    for i, o in enumerate(c.of):                                                  # sqrt: |sqrt x - sqrt y| <= |x - y| / (sqrt x + sqrt y)
        if o.nn_d2 is not None and o.nn_d2.min() > 0:
            assert abs(got['nn_dist_class'][i] - want['nn_dist_class'][i]) <= (o.e_nn / np.sqrt(o.nn_d2)).max(), i
    assert got['intra_precision'] == float(np.nanmean(got['precision_class'])) and got['intra_recall'] == float(np.nanmean(got['recall_class']))
    kd, kw = class_kernel_distance(fa, fb), c.kernel
    assert np.array_equal(np.isnan(kd['kid_class']), np.isnan(kw['kid_class']))          # NaN exactly where a side has fewer than 2 rows
    ok = ~np.isnan(kw['kid_class'])
    q_k = _ratio(np.abs(kd['kid_class'][ok] - kw['kid_class'][ok]), kw['e_kid_class'][ok])
    print('%s: |kid_class - ref| / e_kid %.3e over %d classes' % (name, q_k, ok.sum()))
    _report('kid_%s' % name, q_k)
    assert q_k <= 1.0
    assert kd['intra_kid'] == float(np.nanmean(kd['kid_class'])) and np.array_equal(kd['n_class'], kw['n_class'])


# ----------------------------------------------------------------------------------------------------- segment sums
def test_segment_sums_are_fsum_within_the_any_order_bound_and_repeatable(K):
    lengths = [0, 1, 4097, 0, 300, 256, 257, 0]
    r = np.random.RandomState(5)
    vals = (r.randn(sum(lengths)) * 10.0 ** r.randint(-3, 4, sum(lengths)))
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    v, o = torch.from_numpy(vals).cuda(), torch.from_numpy(off).cuda()
    out = _sentinel(len(lengths), torch.float64, -7.0)
    assert K.segment_sums(v, o, out=out) is out
    got = out.cpu().numpy()
    assert (got[len(lengths):] == -7.0).all()
    for i, n in enumerate(lengths):
        part = vals[off[i]:off[i + 1]]
        assert abs(got[i] - math.fsum(part)) <= max(n - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(part)), i
        if n <= 1:
            assert got[i] == (part[0] if n else 0.0)                            # an empty segment gives 0, one element itself
    assert torch.equal(K.segment_sums(v, o), out[:len(lengths)])                 # a second run: the same bits
    assert K.segment_sums(v, o[:1]).numel() == 0


# ----------------------------------------------------------------------------------------------------- refusals
def test_unsupported_and_bad_arguments_launch_nothing(K):
    f = torch.ones(20, 16, device='cuda')
    seg = torch.tensor([0, 10, 20], dtype=torch.int32, device='cuda')
    out = torch.full((20,), -7.0, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='k = 9'):
        K.knn_radii_seg(f, seg, K.KNN_MAX_K + 1, out=out)
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.knn_radii_seg(torch.ones(20, 1025, device='cuda'), seg, 3, out=out)
    with pytest.raises(ValueError):
        K.knn_radii_seg(f, seg, 0, out=out)
    with pytest.raises(AssertionError):
        K.knn_radii_seg(f, torch.zeros(34, dtype=torch.int32, device='cuda'), 3, out=out)          # 33 classes
    with pytest.raises(AssertionError):
        K.knn_radii_seg(f, seg.long(), 3, out=out)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.knn_radii_seg(f, seg.cpu(), 3, out=out)
    bufs = (torch.full((20,), -3, dtype=torch.int32, device='cuda'), torch.full((20,), -7.0, dtype=torch.float64, device='cuda'),
            torch.full((20,), -5, dtype=torch.int32, device='cuda'))
    r2 = torch.ones(20, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.knn_cover_seg(torch.ones(20, 1025, device='cuda'), seg, torch.ones(20, 1025, device='cuda'), seg, r2, *bufs)
    K.knn_cover_seg(f[:0], seg, f, seg, r2, *bufs)                              # no rows: a successful no-op
    with pytest.raises(AssertionError):
        K.knn_cover_seg(f, seg, f[:, :8].contiguous(), seg, r2, *bufs)
    with pytest.raises(AssertionError):
        K.knn_cover_seg(f, seg, f, seg[:2].contiguous(), r2, *bufs)             # different class counts
    with pytest.raises(AssertionError):
        K.knn_cover_seg(f, seg, f, seg, r2.float(), *bufs)
    with pytest.raises(AssertionError):
        K.knn_cover_seg(f, seg, f, seg, r2, bufs[0][:10], bufs[1], bufs[2])     # an output shorter than m
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.knn_cover_seg(f.cpu(), seg, f, seg, r2, *bufs)
    sums = torch.full(((1 + 2) * (1 + 1),), -7.0, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.kernel_tile_sums_seg(torch.ones(20, 1025, device='cuda'), seg, torch.ones(20, 1025, device='cuda'), seg)
    with pytest.raises(AssertionError, match='exclude_diag'):
        K.kernel_tile_sums_seg(f, seg, f.clone(), seg, exclude_diag=True, out=sums)
    with pytest.raises(AssertionError, match='exclude_diag'):
        K.kernel_tile_sums_seg(f, seg, f, seg.clone(), exclude_diag=True, out=sums)
    with pytest.raises(AssertionError):
        K.kernel_tile_sums_seg(f, seg, f, seg, out=sums[:3])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.kernel_tile_sums_seg(f, seg, f, seg, out=sums.cpu())
    with pytest.raises(AssertionError):
        K.segment_sums(sums.float(), torch.zeros(2, dtype=torch.int64, device='cuda'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.segment_sums(sums, torch.zeros(2, dtype=torch.int64))
    torch.cuda.synchronize()
    assert (out == -7.0).all().item() and (bufs[0] == -3).all().item() and (bufs[1] == -7.0).all().item() and (bufs[2] == -5).all().item()
    assert (sums == -7.0).all().item()


# ----------------------------------------------------------------------------------------------------- end to end
def test_score_generator_with_the_class_references_on_a_resnet_gan(K, clean, monkeypatch):
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import ClassifierScore, FeatureSet
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')          # the classifier trainer's own generator: its names are the GAN's
    scorer = ClassifierScore(tr)
    lab_ref, lab = (np.arange(230) % 10).astype(np.int32), (np.arange(300) % 10).astype(np.int32)
    ref = scorer.features(O.random_images(230, seed=5), chunk=100, labels=lab_ref)
    assert ref.classes == 10 and ref.labels.cpu().tolist() == lab_ref.tolist()
    pooled = FeatureSet(ref.features, ref.classifier)
    case = H.Case(lib, 'resnet', 16, 4, 'cuda')
    try:
        gan = case.trainer()
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        scorer.set_manifold(pooled)
        scorer.set_kernel_reference(pooled)
        plain = scorer.score_generator(gan, 300, labels=lab)
        assert set(plain) == set(SCORE_KEYS) | set(POOLED_KEYS)
        scorer.set_class_manifold(ref)
        scorer.set_class_kernel_reference(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300, labels=lab)
        H.assert_same(before, H.snapshot(lib, gan))
        assert set(got) == set(SCORE_KEYS) | set(POOLED_KEYS) | set(CLASS_KEYS)
        for k in plain:                                                         # no existing key moves by a bit
            assert (got[k] is None and plain[k] is None) or np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        stream.ctr.fill_(c0)
        feats = scorer.features_generator(gan, 300, labels=lab)
        H.assert_same(before, H.snapshot(lib, gan))
        assert feats.classes == 10 and feats.labels.cpu().tolist() == lab.tolist()
        fa, fb = feats.features.cpu().numpy(), ref.features.cpu().numpy()
        of = [CO.ClassOracle(fa[lab == i], fb[lab_ref == i], 3) for i in range(10)]
        want = CO.class_precision_recall(fa, lab, fb, lab_ref, 10, 3, of)
        left, rows = CO.undecidable(of)
        print('resnet generator: precision %s recall %s, oracle %s %s, %d of %d rows undecidable'
              % (got['precision_class'], got['recall_class'], want['precision_class'], want['recall_class'], left, rows))
        assert left <= UNDECIDABLE_CAP * rows
        assert np.array_equal(got['n_class'], want['n_class']) and np.array_equal(got['n_class_reference'], want['n_class_reference'])
        for i, o in enumerate(of):                                              # the counts differ by at most the class's undecidable rows
            assert abs(got['precision_class'][i] - want['precision_class'][i]) * o.m <= (~o.decidable).sum() + 1e-9, i
            assert abs(got['recall_class'][i] - want['recall_class'][i]) * o.n <= (~o.back_decidable).sum() + 1e-9, i
        kw = CO.class_kernel_distance(fa, lab, fb, lab_ref, 10, of)
        assert (np.abs(got['kid_class'] - kw['kid_class']) <= kw['e_kid_class']).all()
        for key, per in (('intra_precision', 'precision_class'), ('intra_recall', 'recall_class'), ('intra_kid', 'kid_class')):
            assert got[key] == float(np.nanmean(got[per])), key
        # the loops' hook logs the three series
        monkeypatch.setitem(evaluate.SCORE_SAMPLES, 'gan_cifar_resnet', 200)
        stream.ctr.fill_(c0)
        series = _Series()
        evaluate.record_score(evaluate.Evaluator(gan), series, scorer)
        stream.ctr.fill_(c0)
        res = scorer.score_generator(gan, 200)
        logged = dict(series.rows)
        assert all(logged[k] == res[k] for k in ('intra_precision', 'intra_recall', 'intra_kid'))
    finally:
        case.close()
