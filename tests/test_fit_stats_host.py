"""not-gpu: the statistics fit (include/gpe_hip_fit.h, ops.FitAccumulator, staging.fit_*) as far as it goes without a device:
  (1) the float64 restatement (tests/fit_stats_restate.py) agrees with the reference's own results in tests/golden/fit_stats_small.pt
      (scripts/make_fit_stats_golden.py): min, max-derived norm_scale bit-equal after fp32 rounding, mean and std within
      n 2^-23 max|x| of the column — the worst case of an fp32 sum of n terms, doubled for the reference's two passes;
  (2) gpe_hip_fit.h parses, its symbols are exported and bound with the parsed types through _lib.FEATURE_HEADERS, the two older
      headers are what they were, and a feature header that declares a missing symbol fails loudly;
  (3) gpe_fit_leaves' values and the entry points' refusals before any launch;
  (4) the Python argument checks that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gpe_amd
from gpe_amd import _lib, ops, staging
import fit_stats_restate as R

FIT = ('gpe_fit_leaves', 'gpe_fit_part', 'gpe_fit_finish')


@pytest.fixture(scope='module')
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, 'fit_stats_small.pt'), weights_only=False)


def _bit_equal(ref, want, what):
    ref = ref.numpy() if torch.is_tensor(ref) else ref
    assert ref.dtype == np.float32 and np.array_equal(ref.view(np.int32), R.f32(want).view(np.int32)), what


def _within(entry, want, bound, what):
    """the reference's fp32 result against the float64 restatement, under the bound recomputed here"""
    d = np.abs(entry['ref'].numpy().astype(np.float64) - want)
    print('%s: |reference - restatement| = %s, bound %s, the generator saw %s' % (what, d, bound, entry['seen'].numpy()))
    assert np.array_equal(entry['bound'].numpy(), bound), what
    assert (entry['seen'].numpy() <= bound).all() and (d <= bound).all(), what


@pytest.mark.parametrize('name', ['padded', 'columns'])
def test_restatement_against_the_reference_cases(fx, name):
    c = fx['cases'][name]
    x = c['x'].numpy()
    w, bound = R.all_stats(x, c['padded']), R.sum_bound(x, c['padded'])
    assert w['n'] == c['n']
    _bit_equal(c['min'], w['min'], name)
    _bit_equal(c['norm_scale'], w['norm_scale'], name)
    _within(c['mean'], w['mean'], bound, name + ' mean')
    _within(c['std'], w['std'], bound, name + ' std')


def test_the_cases_are_the_ones_that_matter(fx):
    pad, col = fx['cases']['padded'], fx['cases']['columns']
    x = pad['x'].numpy()
    assert x.shape == (3, 4, 6, 4) and (x.reshape(3, 4, -1) == 0).all(axis=2).any()              # whole empty panels
    assert (x[0, 0, 1] == 0).all() and (x[0, 0, 0] != 0).any() and (x[0, 0, 2] != 0).any()       # a zero row inside a loop
    assert 0 < np.abs(x[0, 1, 0]).max() <= 5.1e-6 and 1.9e-5 <= np.abs(x[0, 1, 1]).max() <= 2.1e-5
    kept = R.unpad(x)
    assert pad['n'] == len(kept) and any((r == x[0, 1, 1]).all() for r in kept) and not any((r == x[0, 1, 0]).all() for r in kept)
    y = col['x'].numpy().reshape(-1, 6)
    assert (y[:, 0] == 0.75).all() and (y[:, 1] == 0).all() and (y[:, 3] == -2.5).all()
    assert 0 < y[:, 2].max() - y[:, 2].min() < 2e-6 and y[:, 2].min() == 1.0
    assert col['norm_scale'].tolist()[:4] == [0.75, 1.0, 1.0, -2.5]
    assert col['std']['ref'].tolist()[0] == 0.0 and col['std']['ref'].tolist()[1] == 0.0 and col['std']['ref'].tolist()[3] == 0.0
    assert float(col['norm_scale'][4]) == float(np.float32(y[:, 4].max()) - np.float32(y[:, 4].min()))


def test_restatement_against_the_two_standardize_methods(fx):
    p = fx['pattern']
    feats, gt = p['features'].numpy(), {k: v.numpy() for k, v in p['gt'].items()}
    assert feats.shape[0] * feats.shape[1] <= 2000
    w = R.pattern_standardize(feats, gt)
    _within(p['f_shift'], w['f_shift'], R.sum_bound(feats), 'f_shift')
    _within(p['f_scale'], w['f_scale'], R.sum_bound(feats), 'f_scale')
    _within(p['gt_shift']['outlines'], w['gt_shift']['outlines'], R.sum_bound(gt['outlines'], True), 'outlines shift')
    _within(p['gt_scale']['outlines'], w['gt_scale']['outlines'], R.sum_bound(gt['outlines'], True), 'outlines scale')
    assert p['gt_shift']['outlines']['ref'].tolist()[:2] == [0.0, 0.0] and w['gt_shift']['outlines'][:2].tolist() == [0.0, 0.0]
    for k in ('rotations', 'translations', 'stitch_tags'):
        _bit_equal(p['gt_shift'][k], w['gt_shift'][k], k)
        _bit_equal(p['gt_scale'][k], w['gt_scale'][k], k)
    s = fx['stitch']
    w = R.stitch_standardize(s['features'].numpy())
    _bit_equal(s['f_shift'], w['f_shift'], 'stitch f_shift')
    _bit_equal(s['f_scale'], w['f_scale'], 'stitch f_scale')


def test_scale_rule():
    assert R.scale_rule(0.75, 0.75) == 0.75 and R.scale_rule(0.0, 0.0) == 1.0 and R.scale_rule(-2.5, -2.5) == -2.5
    assert R.scale_rule(1.0, np.float32(1.000001)) == 1.0 and R.scale_rule(1.0, 1.5) == 0.5
    assert R.scale_rule(5e-9, 8e-9) == 1.0 and R.scale_rule(-1.0, 3.0) == 4.0
    assert np.isnan(R.scale_rule(np.nan, np.nan))


def test_the_fit_header_is_bound_and_exported():
    main, ext, fit = _lib.parse_header(), _lib.parse_header(_lib.EXT_HEADER_PATH), _lib.parse_header(_lib.FIT_HEADER_PATH)
    assert set(fit) == set(FIT) and not set(fit) & (set(main) | set(ext))
    # the two older headers and the tuple the older tests pin are what they were
    assert len(main) == 123 and set(ext) == {'gpe_grad_norm_slots', 'gpe_grad_norm_part', 'gpe_grad_norm_finish', 'gpe_adam_step_guarded',
                                             'gpe_adam_step_guarded_dev'}
    assert _lib.HEADERS == (_lib.HEADER_PATH, _lib.EXT_HEADER_PATH) and _lib.FEATURE_HEADERS == (_lib.FIT_HEADER_PATH,)
    assert fit['gpe_fit_leaves'] == ('l', ['l', 'l'])
    assert fit['gpe_fit_part'] == ('i', ['p', 'l', 'l', 'i', 'i', 'l', 'l', 'p', 'p'])
    assert fit['gpe_fit_finish'] == ('i', ['p', 'l', 'i', 'p', 'p'])
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in fit:
        assert hasattr(raw, name), 'libgpe_hip.so does not export %s' % name
    l = _lib.lib()
    assert l.gpe_abi_version() == 7
    for name, (res, args) in fit.items():
        fn = getattr(l, name)
        assert fn.restype is _lib._CT[res] and list(fn.argtypes) == [_lib._CT[a] for a in args], name


def test_a_feature_symbol_that_is_not_exported_fails_loudly(tmp_path, monkeypatch):
    h = tmp_path / 'feature.h'
    h.write_text('int gpe_fit_not_in_the_library(const float* x, void* stream);\n')
    monkeypatch.setattr(_lib, 'FEATURE_HEADERS', (_lib.FIT_HEADER_PATH, str(h)))
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(AttributeError, match='gpe_fit_not_in_the_library'):
        _lib.lib()


def test_leaves_is_host_only():
    l = _lib.lib()
    for sets, rows, want in ((1, 1, 1), (1, 512, 1), (1, 513, 2), (3, 1025, 9), (300, 23, 300), (5000, 2000, 20000),
                             (2 ** 40, 2 ** 31, 2 ** 62)):
        assert l.gpe_fit_leaves(sets, rows) == want == ops.fit_leaves(sets, rows)
    for sets, rows in ((0, 5), (5, 0), (-1, 5), (5, -1), (2 ** 62, 513), (2 ** 41, 2 ** 31 + 1)):
        assert l.gpe_fit_leaves(sets, rows) == -22
        with pytest.raises(ValueError, match='fit_leaves'):
            ops.fit_leaves(sets, rows)


def test_bad_arguments_are_rejected_without_a_gpu():
    """The non-NULL 'device' pointers are made-up addresses: an entry point that refuses its arguments never touches them."""
    l = _lib.lib()
    A = 0x7f0000001000
    part = lambda **k: l.gpe_fit_part(*[k.get(n, d) for n, d in (('x', A), ('sets', 3), ('rows', 600), ('C', 3), ('skip', 0), ('leaf0', 0),
                                                                  ('total', 6), ('part', A), ('stream', None))])
    for bad in (dict(x=None), dict(part=None), dict(x=A + 2), dict(part=A + 4), dict(C=0), dict(C=17), dict(sets=0), dict(rows=0),
                dict(sets=-3), dict(leaf0=-1), dict(leaf0=1), dict(total=5), dict(total=0), dict(sets=2 ** 40, rows=2 ** 30, total=2 ** 62),
                dict(leaf0=2 ** 62, total=2 ** 62)):
        assert part(**bad) == -22, bad
    fin = lambda **k: l.gpe_fit_finish(*[k.get(n, d) for n, d in (('part', A), ('leaves', 6), ('C', 3), ('result', A), ('stream', None))])
    for bad in (dict(part=None), dict(result=None), dict(part=A + 4), dict(result=A + 4), dict(leaves=0), dict(leaves=-1), dict(C=0),
                dict(C=17), dict(leaves=2 ** 62)):
        assert fin(**bad) == -22, bad


def test_accumulator_checks_need_no_device():
    for bad in (0, 17, -1, 3.0, True, None):
        with pytest.raises(ValueError, match='columns'):
            ops.FitAccumulator(bad, 4, 100, 'cuda')
    for kw in (dict(sets=0), dict(sets=-2), dict(sets=2.0), dict(rows_per_set=0), dict(rows_per_set=True)):
        with pytest.raises(ValueError, match='positive integer'):
            ops.FitAccumulator(3, **{'sets': 4, 'rows_per_set': 100, 'device': 'cuda', **kw})
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.FitAccumulator(3, 4, 100, 'cpu')
    x = torch.zeros(2, 100, 3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fit_part(x, torch.zeros(2, 13, dtype=torch.float64))
    with pytest.raises(ValueError, match=r'\[S, N, C\]'):
        ops.fit_part(torch.zeros(100, 3), torch.zeros(2, 13, dtype=torch.float64))
    with pytest.raises(ValueError, match='part must be'):
        ops.fit_finish(torch.zeros(2, 13))
    with pytest.raises(ValueError, match='part must be'):
        ops.fit_finish(torch.zeros(2, 12, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fit_finish(torch.zeros(2, 13, dtype=torch.float64))


def test_fit_read_rounds_once_and_refuses_an_empty_fit():
    C = 2
    block = torch.tensor([7.0, 2.0] + [0.1, 1.0 + 2.0 ** -30] + [0.5, 0.0] + [-1.0, 3.0] + [2.0, 3.0] + [3.0, 1.0], dtype=torch.float64)
    r = ops.fit_read(block)
    assert r['n'] == 7 and r['status'] == ops.FIT_STATUS_NONFINITE and set(r) == {'n', 'status', 'mean', 'std', 'min', 'max', 'norm_scale'}
    assert all(r[k].dtype == np.float32 and r[k].shape == (C,) for k in ('mean', 'std', 'min', 'max', 'norm_scale'))
    assert r['mean'].tolist() == [float(np.float32(0.1)), 1.0] and r['norm_scale'].tolist() == [3.0, 1.0]
    empty = torch.tensor([0.0, 1.0] + [float('nan')] * (5 * C), dtype=torch.float64)
    with pytest.raises(ValueError, match='no row'):
        ops.fit_read(empty)


def test_staging_checks_need_no_device():
    gt = {'outlines': torch.zeros(2, 3, 4, 4), 'rotations': torch.zeros(2, 3, 4), 'translations': torch.zeros(2, 3, 3),
          'stitch_tags': torch.zeros(2, 3, 4, 3)}
    fs = {'f_shift': [0, 0, 0], 'f_scale': [1, 1, 1]}
    with pytest.raises(ValueError, match='ground_truth must hold'):
        staging.fit_pattern_standardization({k: v for k, v in gt.items() if k != 'rotations'}, fs)
    with pytest.raises(ValueError, match='feature_stats'):
        staging.fit_pattern_standardization(gt, {'f_shift': [0, 0, 0]})
    with pytest.raises(ValueError, match='outlines'):
        staging.fit_pattern_standardization({**gt, 'outlines': torch.zeros(2, 12, 4)}, fs)
    with pytest.raises(ValueError, match='rotations'):
        staging.fit_pattern_standardization({**gt, 'rotations': torch.zeros(2, 3, 4, dtype=torch.float64)}, fs)
    with pytest.raises(ValueError, match='garments'):
        staging.fit_pattern_standardization({**gt, 'translations': torch.zeros(3, 3, 3)}, fs)
    with pytest.raises(RuntimeError, match='no CPU path'):
        staging.fit_pattern_standardization(gt, fs)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='chunk'):
            staging._fit_chunk(bad)
    for bad in ([], [0.5, 1.0], [[0, 1]], torch.tensor([True])):
        with pytest.raises(ValueError, match='index'):
            staging._fit_index(bad, 'cpu')
    assert staging._fit_index([2, 0, 1], 'cpu').tolist() == [2, 0, 1]
    assert hasattr(staging.MeshPointSampler, 'fit_feature_stats') and hasattr(staging.StitchPairSampler, 'fit_feature_stats')
    assert gpe_amd.staging is staging
