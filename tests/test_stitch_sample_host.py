"""not-gpu: the host restatement of the training-pair sampler (tests/stitch_sample_restate.py, the yardstick of
tests/test_gpu_stitch_sample.py) — Philox4x32-10 against Random123's known answers, its distribution and the reference's recorded
counts (tests/golden/stitch_sample_small.pt, scripts/make_stitch_sample_golden.py) against the analytic model of
NNSewingPattern.stitches_as_3D_pairs, its invariants on the six stitch_pairs_* garments — and the argument checks of
gpe_stitch_sample / ops.stitch_pairs_sample, which need no GPU.

The statistical bars are the 0.9999 chi-square quantiles (Wilson-Hilferty) of the five statistics of chi2_statistics; both sides
are deterministic (recorded counts; fixed seeds), so a test either always passes or always fails."""
import ctypes
import os

import numpy as np
import pytest
import torch

import stitch_sample_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')


@pytest.fixture(scope='module')
def recorded():
    return torch.load(os.path.join(GOLDEN, 'stitch_sample_small.pt'), weights_only=False)


@pytest.fixture(scope='module')
def garments():
    return R.resident_set(GOLDEN)


def _slot(gs, tag):
    g = gs['tags'].index(tag)
    return gs['edges'][g], gs['num_edges'][g], gs['gt'][g], gs['gt_num'][g]


def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    ctr = np.asarray([c[0] for c in cases], dtype=np.uint32)
    key = np.asarray([c[1] for c in cases], dtype=np.uint32)
    out = R.philox4x32(ctr, key)                           # vectorised, as the sampler calls it
    for row, (_, _, want) in zip(out, cases):
        assert ' '.join('%08x' % v for v in row) == want
    # the counter layout of a decision: item | kind << 28, attempt | b << 8, draw lo, draw hi; key = seed lo, seed hi
    seed, draw = 0x299f31d0a4093822, 0x0370734413198a2e
    w = R.words(2, 0x043f6a88, 0x85a308, seed, draw, attempt=0xd3)
    assert ' '.join('%08x' % v for v in w) == cases[2][2]
    assert R.below(np.uint32(0xffffffff), 7) == 6 and R.below(np.uint32(0), 7) == 0 and R.below(np.uint32(1 << 31), 5) == 2


def test_quantile_approximation():
    # tabulated chi-square quantiles; Wilson-Hilferty is within 0.3 % at these degrees of freedom
    for df, p, want in ((23, 0.99, 41.638), (225, 0.99, 277.27), (497, 0.99, 573.25), (23, 0.9999, 57.28)):
        assert abs(R.chi2_quantile(df, p) - want) < 3e-3 * want, (df, p, R.chi2_quantile(df, p))


def _under_the_bar(stats):
    for k, (x, df) in stats.items():
        bar = R.chi2_quantile(df, 0.9999)
        print('%-8s chi-square %9.2f on %3d degrees of freedom, bar %9.2f' % (k, x, df, bar))
        assert x < bar, k


def test_recorded_reference_counts_follow_the_analytic_model(recorded, garments):
    edges, ne, gt, num = _slot(garments, 'small')
    L = edges.shape[1]
    st = R.valid_stitches(ne, L, gt, num)
    small_L = 6                                            # the fixture's ids are panel * 6 + edge (its own, unpadded layout)
    to_set = lambda e: (e // small_L) * L + e % small_L
    assert [(to_set(int(a)), to_set(int(b))) for a, b in recorded['stitches'].tolist()] == st
    assert recorded['flip_inconsistent'] == 0 and recorded['N'] >= 1700
    rec = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in recorded.items()}
    ne_small = ne[:8]
    _under_the_bar(R.chi2_statistics(rec, ne_small, small_L, [tuple(s) for s in recorded['stitches'].tolist()],
                                     recorded['n_stitched'], recorded['n_non_stitched']))


def test_restatement_follows_the_analytic_model(recorded, garments):
    edges, ne, gt, num = _slot(garments, 'small')
    P, L, _ = edges.shape
    st = R.valid_stitches(ne, L, gt, num)
    n_st, n_non, N = recorded['n_stitched'], recorded['n_non_stitched'], recorded['N']
    dec = [R.sample(edges, ne, gt, num, d % 3, n_st, n_non, 3, garments['shift'], garments['scale'], 0x5eed0001cafe0000 + d // 1000, d)
           for d in range(N)]
    assert all(d['status'] == 0 for d in dec)
    _under_the_bar(R.chi2_statistics(R.tally(dec, P * L, st, n_st, n_non), ne, L, st, n_st, n_non))


@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('tag', R.TAGS)
def test_restatement_invariants(garments, tag, flags):
    edges, ne, gt, num = _slot(garments, tag)
    L = edges.shape[1]
    Sv = len(R.valid_stitches(ne, L, gt, num))
    for n_st, n_non in ((Sv, 1), (Sv + 3, 9)):
        if n_st + n_non == 0:
            continue
        d = R.sample(edges, ne, gt, num, 2, n_st, n_non, flags, garments['shift'], garments['scale'], 7 << 40, 5)
        R.check_slot(d['rows'], d['labels'], d['status'], edges, ne, gt, num, n_st, n_non, flags, garments['shift'], garments['scale'])
        assert d['status'] == 0 and sorted(d['perm'].tolist()) == list(range(n_st + n_non))
        assert (d['perm'] == np.arange(n_st + n_non)).all() or flags & 2
        if Sv == 0:
            assert not d['labels'].any() and len(d['pairs']) == n_st + n_non         # all R rows are non-stitched
        else:
            assert len(d['pairs']) == n_non and len(d['choices']) == n_st - Sv and all(0 <= c < Sv for c in d['choices'])


def test_status_paths(garments):
    edges, ne, gt, num = _slot(garments, 'small')
    sh, sc = garments['shift'], garments['scale']
    d = R.sample(edges, ne, gt, num, 0, 3, 5, 3, sh, sc, 1, 0)                       # four valid stitches, three asked for
    assert d['status'] == -1 and not d['rows'].any() and not d['labels'].any()
    # entries naming an absent edge are skipped (the reference's IndexError branch): panel 1 is absent, edge 5 of panel 0 too
    L = edges.shape[1]
    gt2 = gt.copy()
    gt2[:, 1] = (1 * L + 0, 2 * L + 1)
    gt2[:, 2] = (0 * L + 5, 2 * L + 1)
    assert len(R.valid_stitches(ne, L, gt2, num)) == 2
    d = R.sample(edges, ne, gt2, num, 0, 3, 5, 3, sh, sc, 1, 0)
    assert d['status'] == 0 and d['labels'].sum() == 3
    R.check_slot(d['rows'], d['labels'], d['status'], edges, ne, gt2, num, 3, 5, 3, sh, sc)
    # one present edge: every attempt is a self pair; a row gives up after exactly 64 and the call returns
    one = np.zeros_like(ne)
    one[3] = 1
    d = R.sample(edges, one, gt, 0, 0, 2, 4, 3, sh, sc, 1, 0)
    assert d['status'] == 6 and d['attempts'] == [R.ATTEMPTS] * 6 and not d['rows'].any() and not d['labels'].any()
    d = R.sample(edges, one, gt, 0, 0, 0, 4, 3, sh, sc, 1, 0)
    assert d['status'] == 4 and d['attempts'] == [R.ATTEMPTS] * 4
    # an index outside the set
    rows, labels, status, _ = R.sample_batch(garments['edges'], garments['num_edges'], garments['gt'], garments['gt_num'], [-1, 0, 6],
                                             6, 4, 3, sh, sc, 1, 0)
    assert status.tolist() == [-2, 0, -2] and not rows[[0, 2]].any() and rows[1].any()


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from gpe_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    good = dict(edges=p, ne=p, gt=p, num=p, G=1, P=4, L=4, Fe=8, S=2, index=p, B=1, n_st=2, n_non=2, flags=3, sh=p, sc=p, state=p,
                ticket=p, rows=p, labels=p, status=p)

    def call(**kw):
        a = dict(good, **kw)
        return l.gpe_stitch_sample(a['edges'], a['ne'], a['gt'], a['num'], a['G'], a['P'], a['L'], a['Fe'], a['S'], a['index'], a['B'],
                                   a['n_st'], a['n_non'], a['flags'], a['sh'], a['sc'], a['state'], a['ticket'], a['rows'], a['labels'],
                                   a['status'], None)
    for name in ('edges', 'ne', 'gt', 'num', 'index', 'sh', 'sc', 'state', 'ticket', 'rows', 'labels', 'status'):
        assert call(**{name: None}) == -22, name
    assert call(Fe=17) == -22 and call(Fe=0) == -22
    assert call(Fe=6) == -22 and call(Fe=6, flags=1) == -22            # the flip needs the 8-feature layout
    assert call(flags=4) == -22
    assert call(P=33, L=16) == -22 and call(P=513, L=1) == -22         # P L > 512
    assert call(n_st=0, n_non=0) == -22 and call(n_st=4096, n_non=1) == -22 and call(n_st=-1, n_non=3) == -22
    assert call(B=0) == -22 and call(G=0) == -22 and call(S=-1) == -22


def test_op_has_no_cpu_path_and_checks_its_arguments(garments):
    import gpe_amd
    gs = garments
    t = lambda k, dt=torch.int64: torch.from_numpy(gs[k]).to(dt)
    args = [t('edges', torch.float32), t('num_edges'), t('gt'), t('gt_num'), torch.tensor([0, 1]), 6, 4, gs['shift'], gs['scale'],
            torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)]
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe_amd.ops.stitch_pairs_sample(*args)
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe_amd.staging.StitchPairSampler(*args[:4], {'f_shift': gs['shift'], 'f_scale': gs['scale']})
    for i, bad in ((0, args[0][0]), (1, args[1].float()), (2, args[2][:, :1]), (3, args[3][:-1])):
        with pytest.raises(ValueError):
            gpe_amd.ops.stitch_pairs_sample(*(args[:i] + [bad] + args[i + 1:]))
    with pytest.raises(ValueError, match='512'):
        gpe_amd.ops.stitch_pairs_sample(torch.zeros(1, 33, 16, 8), *args[1:])
