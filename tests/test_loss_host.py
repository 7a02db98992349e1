"""not-gpu: the restated pattern / stitch loss kernels, the renumbering and the panel shift of tests/loss_restate.py are checked
before any GPU time is spent on them.
  (1) the closed-form restatements (which carry the variants) agree with the oracle's classes and with torch's own fp64 mse_loss /
      binary_cross_entropy_with_logits and their autograd at 1e-12 on every case; the kernels' convention at a gap of exactly 0
      differs from the reference in the case built for it only, by the full (HardNet) / half (all-pairs) gradient of that pair;
  (2) every stitch case satisfies the input conditions (|margin - d| and the separation of the two smallest distances at least
      2^-16 max(1, d), or exact on the grid): none is left out; the structured cases hold the ties they were built for;
  (3) the unmodified reference passes its own checker, rounded once to fp32; the shared cases stay unchanged;
  (4) every entry of VARIANTS is rejected by at least one case of its kernel at ten times the bar of the GPU test;
  (5) the C ABI without a device: the six symbols are declared and exported, -22 for every rejected argument."""
import ctypes

import numpy as np
import pytest
import torch

import loss_restate as R


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all()
    ok = ~np.isnan(a)
    return float((np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok]))).max()) if ok.any() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# (1) the restatements are the reference's operation
# ----------------------------------------------------------------------------------------------------------------------
def test_stitch_restatement_agrees_with_the_oracle():
    worst = 0.0
    for case in R.cases('stitch_loss_fwd'):
        want = R.oracle_stitch(case)
        got = R.restate_stitch(case, conv='reference')
        kern = R.restate_stitch(case, conv='kernel')
        for k in ('out5', 'sim_b', 'g_tags', 'g_mask'):
            e = _close(got[k], want[k])
            worst = max(worst, e)
            assert e <= 1e-12, (case.id, k, e)
            assert _close(kern[k], want[k]) <= 1e-12 or (case.kind == 'gap0' and k == 'g_tags'), (case.id, k)
        assert np.isfinite(want['g_tags']).all() and np.isfinite(want['g_mask']).all(), case.id
    print('stitch restatement against the oracle: worst %.2e over %d cases' % (worst, len(R.cases('stitch_loss_fwd'))))


def test_gap_of_exactly_zero_is_the_only_difference_in_convention():
    """the reference's autograd sends the pair's full gradient (HardNet) or half of it (all-pairs) at margin - d == 0, the
    kernels none: the values agree, and the gradients differ on the two edges of that pair alone, by exactly that amount"""
    seen = 0
    for case in R.cases('stitch_loss_bwd'):
        if case.kind != 'gap0':
            continue
        seen += 1
        p = case.p
        ref, kern = R.oracle_stitch(case), R.restate_stitch(case, conv='kernel')
        assert _close(ref['out5'], kern['out5']) <= 1e-12 and ref['out5'][2] == 0.0
        diff = ref['g_tags'] - kern['g_tags']
        assert (diff[1] == 0).all() and (diff[0, 2:] == 0).all()
        t = case.v64('tags').reshape(p['B'], -1, p['D'])[0]
        gs = 1.0 if p['gscale'] is None else p['gscale']
        ntot = 2 * sum(p['nums'])
        # d/dt_0 of -(|t_0 - t_1|^2): once under HardNet from each end's own minimum = 2 ends; all-pairs: 2 ends / (2 n), halved
        share = 2.0 / ntot if p['flags'] & 2 else 0.5 * 2.0 / (2 * p['nums'][0] * ntot)
        want = -2 * (t[0] - t[1]) * share * gs
        assert np.abs(diff[0, 0] - want).max() <= 1e-12 and np.abs(diff[0, 1] + want).max() <= 1e-12, (case.id, diff[0, :2], want)
    assert seen == 2


def test_pattern_restatement_agrees_with_the_oracle():
    worst = 0.0
    for case in R.cases('pattern_loss_fwd'):
        want, got = R.oracle_pattern(case), R.restate_pattern(case)
        for k in want:
            e = _close(got[k], want[k])
            worst = max(worst, e)
            assert e <= 1e-12, (case.id, k, e)
        ne = case.inp['num_edges']
        if ne.size >= 6:
            assert set(ne.tolist()) == {-1, 0, 2, 3, case.p['L'], case.p['L'] + 5}, case.id
    print('pattern restatement against torch mse_loss + PanelLoopLoss: worst %.2e' % worst)


def test_references_agree_with_torch_on_the_dense_cases():
    """plain fp64 MSE and BCE terms against torch.nn.functional and its autograd at 1e-12, where the views are dense"""
    n = 0
    for case in R.cases('stitch_loss_fwd'):
        p = case.p
        if p['layout'] != 'dense' or p['flags'] & 1 or not p['flags'] & 12:
            continue
        n += 1
        got = R.restate_stitch(case)
        gs = 1.0 if p['gscale'] is None else p['gscale']
        if p['flags'] & 4:
            x = torch.tensor(case.inp['logit_buf'], dtype=torch.float64).requires_grad_()
            f = torch.nn.functional.binary_cross_entropy_with_logits(x, torch.tensor(case.inp['gt_mask'], dtype=torch.float64))
            (f * gs).backward()
            assert abs(got['out5'][4] - f.item()) <= 1e-12 and np.abs(got['g_mask'].reshape(x.shape) - x.grad.numpy()).max() <= 1e-12
        if p['flags'] & 8:
            t = torch.tensor(case.inp['tags_buf'], dtype=torch.float64).requires_grad_()
            f = torch.nn.functional.mse_loss(t, torch.tensor(case.inp['gt_tags'], dtype=torch.float64))
            (f * gs * p['sup_w']).backward()
            assert abs(got['out5'][3] - f.item()) <= 1e-12 and np.abs(got['g_tags'].reshape(t.shape) - t.grad.numpy()).max() <= 1e-12
    assert n >= 2


def test_integer_restatements_agree_with_the_oracle():
    for kernel, restate in (('stitch_renumber', R.restate_renumber), ('panel_shift', R.restate_shift)):
        for case in R.cases(kernel):
            want = restate(case)
            got = restate(case, variant='none')                  # the hand-written loop with no mistake switched on
            assert np.array_equal(got, want), (kernel, case.id)


# ----------------------------------------------------------------------------------------------------------------------
# (2) conditions on the inputs; the case lists are the issue's
# ----------------------------------------------------------------------------------------------------------------------
def test_every_stitch_case_is_within_the_input_conditions():
    cases = R.cases('stitch_loss_fwd')
    left_out = []
    for case in cases:
        p = case.p
        if p['flags'] & 1 and not R._conditions(case.v64('tags').reshape(p['B'], -1, p['D']), p['st_clean'], p['nums'], p['margin'], case.grid):
            left_out.append(case.id)
    print('%d stitch cases, %d left out; seeds tried beyond the first: %d' % (len(cases), len(left_out), sum(c.seed for c in cases)))
    assert left_out == []
    assert len(cases) == 16 + 4 * 6 + sum(len(f) for f in R.GRID_KINDS.values())


def _min_ties(case):
    """per tag of pattern 0: (number of tags at the HardNet minimum, number of distinct edges among them, active)"""
    p = case.p
    n = p['nums'][0]
    t = case.v64('tags').reshape(p['B'], -1, p['D'])[0]
    edges = np.concatenate([p['st_clean'][0, 0, :n], p['st_clean'][0, 1, :n]])
    T = t[edges]
    d = ((T[:, None] - T[None]) ** 2).sum(-1)
    idx = np.arange(2 * n)
    d[idx, idx] = d[idx, (idx + n) % (2 * n)] = np.inf
    out = []
    for i in idx:
        at = np.flatnonzero(d[i] == d[i].min())
        out.append((len(at), len(set(edges[at].tolist())), p['margin'] - d[i].min() > 0))
    return out, edges


def test_structured_cases_hold_what_they_were_built_for():
    by = {}
    for case in R.cases('stitch_loss_fwd'):
        if case.grid:
            by.setdefault(case.kind, case)
    assert set(by) == set(R.GRID_KINDS)
    ties, edges = _min_ties(by['dup2'])
    assert np.bincount(edges).max() == 2 and (2, 1, True) in ties        # one edge, two identical tags, an active tied minimum
    ties, edges = _min_ties(by['dup3'])
    assert np.bincount(edges).max() == 3 and (3, 1, True) in ties
    assert (2, 2, True) in _min_ties(by['tie2'])[0] and (3, 3, True) in _min_ties(by['tie3'])[0]
    t = by['same'].v64('tags')[0]
    assert (t == t[0, 0]).all()
    assert R.expected(by['far'])['out5'][2] == 0.0 and R.expected(by['gap0'])['out5'][2] == 0.0
    raw, PL = by['clamp'].inp['stitches'][0, :, :3], by['clamp'].p['P'] * by['clamp'].p['L']
    assert raw.min() < 0 and raw.max() >= PL and np.array_equal(by['clamp'].p['st_clean'][0, :, :3], np.clip(raw, 0, PL - 1))
    # on the grid every squared distance is a multiple of 1/64: exact in fp32 in any order
    for case in by.values():
        assert (case.v64('tags') * 8 == np.round(case.v64('tags') * 8)).all() and case.p['margin'] == 0.5


def test_case_lists_cover_the_issue():
    assert set(R.VARIANTS) == set(R.KERNELS) == set(R.GROUP)
    st = R.cases('stitch_loss_fwd')
    assert {c.p['flags'] for c in st if c.id.startswith('3-2-4-3-3-')} == set(range(16))
    assert {(c.p['layout'], c.p['gscale']) for c in st} == {(l, g) for l in R.LAYOUTS for g in R.GSCALES}
    assert any(not c.p['g_mask'] and c.p['g_tags'] for c in st) and any(not c.p['g_tags'] and c.p['g_mask'] for c in st)
    pt = R.cases('pattern_loss_fwd')
    assert {c.p['flags'] for c in pt if c.id.startswith('3-2-4-1-5-')} == set(range(16)) and len(pt) == 16 + 4 * 3
    assert {(c.p['layout'], c.p['gscale']) for c in pt} == {(l, g) for l in R.LAYOUTS for g in R.GSCALES}
    assert {c.p['pad'] for c in pt} == {(0.0, 0.0), (0.375, -1.25)} and len({c.p['loop_w'] for c in pt}) == 2
    assert any(not c.p['g_rot'] for c in pt) and any(not c.p['g_tr'] for c in pt) and any(c.p['g_rot'] and c.p['g_tr'] for c in pt)
    rn = R.cases('stitch_renumber')
    assert {c.p['S'] for c in rn} == {1, 5, 64, 70}
    seen = set()
    for c in rn:
        S = c.p['S']
        seen |= {'zero' if n == 0 else 'full' if n == S else 'above' if n > S else 'negative' if n < 0 else 'part' for n in c.inp['nums']}
    assert seen >= {'zero', 'full', 'above', 'negative'}
    sh = R.cases('panel_shift')
    assert {(c.p['npanels'], c.p['L'], c.p['D']) for c in sh} == {(n, L, D) for n in (1, 7, 46) for L in (3, 14) for D in (1, 3)}
    assert any((c.inp['lead'] >= c.p['L']).any() for c in sh)          # num_edges = L + 5 with lead = n - 1: past the panel's rows
    for c in sh:
        assert {0, 1} <= set(c.inp['lead'].tolist()) or c.p['npanels'] == 1
        if c.p['npanels'] >= 7:
            L = c.p['L']
            assert set(c.inp['num_edges'].tolist()) == {0, 2, 3, L, L + 5}, c.id


# ----------------------------------------------------------------------------------------------------------------------
# (3) every bar passes its own reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', R.KERNELS)
def test_bar_accepts_its_reference(kernel):
    worst = {}
    for case in R.cases(kernel):
        before = {n: a.tobytes() for n, a in case.inp.items()}
        outs = {n: a.tobytes() for n, a in case.out0[kernel].items()}
        for k, v in R.check(case, kernel, R.emulate(case, kernel)).items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert all(case.inp[n].tobytes() == b for n, b in before.items()) and all(case.out0[kernel][n].tobytes() == b for n, b in outs.items())
    print('%s: the reference rounded to fp32, worst in bars: %s' % (kernel, ', '.join('%s %.3f' % kv for kv in sorted(worst.items())) or 'exact'))


def test_checker_rejects_a_touched_sentinel_a_nan_and_a_nonzero_zero():
    case = next(c for c in R.cases('stitch_loss_bwd') if c.id.startswith('3-2-4-3-3-f15'))
    good = R.emulate(case, 'stitch_loss_bwd')
    R.check(case, 'stitch_loss_bwd', good)
    n = case.p['B'] * case.p['P'] * case.p['L'] * case.p['D']
    for at, v in ((n, 0.0), (0, np.nan)):
        bad = {k: a.copy() for k, a in good.items()}
        bad['g_tags'][at] = v
        with pytest.raises(AssertionError):
            R.check(case, 'stitch_loss_bwd', bad)
    hard = next(c for c in R.cases('stitch_loss_bwd') if c.id.startswith('3-2-4-3-3-f3-'))      # no supervised term: pattern 2 (n = 0) is all 0
    good = R.emulate(hard, 'stitch_loss_bwd')
    assert (good['g_tags'][2 * n // 3:n] == 0).all()
    good['g_tags'][n - 1] = 1e-30
    with pytest.raises(AssertionError, match='exactly 0'):
        R.check(hard, 'stitch_loss_bwd', good)
    fwd = R.emulate(case, 'stitch_loss_fwd')
    assert np.isnan(fwd['out5'][0]) and np.isnan(fwd['out5'][1]) and np.isfinite(fwd['out5'][2:5]).all()
    fwd['out5'][0] = 1.0
    with pytest.raises(AssertionError):
        R.check(case, 'stitch_loss_fwd', fwd)


# ----------------------------------------------------------------------------------------------------------------------
# (4) every bar discriminates
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', R.KERNELS)
def test_every_variant_is_rejected(kernel):
    assert R.VARIANTS[kernel]
    emu = [(case, R.emulate(case, kernel)) for case in R.cases(kernel)]
    for variant in R.VARIANTS[kernel]:
        rejecting = []
        for case, got in emu:
            try:
                R.check(case, kernel, got, variant=variant, scale=10.0)
            except AssertionError:
                rejecting.append(case.id)
        print('%s / %s: rejected at ten bars by %d of %d cases: %s' % (kernel, variant, len(rejecting), len(emu), ', '.join(rejecting[:6])))
        assert rejecting, 'no case of %s tells the variant %r from the kernel' % (kernel, variant)


# ----------------------------------------------------------------------------------------------------------------------
# (5) the C ABI without a device
# ----------------------------------------------------------------------------------------------------------------------
SYMBOLS = ('gpe_pattern_loss_fwd', 'gpe_pattern_loss_bwd', 'gpe_stitch_loss_fwd', 'gpe_stitch_loss_bwd', 'gpe_stitch_renumber',
           'gpe_panel_shift')


def test_header_declares_and_library_exports_the_symbols():
    from gpe_amd import _lib
    sigs = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in sigs and hasattr(raw, name), name
        assert sigs[name][0] == 'i' and sigs[name][1][-1] == 'p'
    st = 'p' + 'lll' + 'i' + 'p' + 'lll' + 'pp' + 'i' + 'pp' + 'iiii' + 'ff'
    pt = 'p' + 'lll' + 'pl' + 'pl' + 'pppp' + 'iiiiii' + 'fff'
    assert sigs['gpe_stitch_loss_fwd'][1] == list(st + 'pp') + ['p'] and sigs['gpe_stitch_loss_bwd'][1] == list(st + 'pppp') + ['p']
    assert sigs['gpe_pattern_loss_fwd'][1] == list(pt + 'ppp') + ['p'] and sigs['gpe_pattern_loss_bwd'][1] == list(pt + 'ppppp') + ['p']
    assert sigs['gpe_stitch_renumber'][1] == list('pp' + 'iiii' + 'pppp') + ['p'] and sigs['gpe_panel_shift'][1] == list('pippli' + 'p') + ['p']


def _swap(args, **kw):
    out = dict(args)
    out.update(kw)
    return list(out.values())


def test_bad_arguments_are_rejected_without_a_gpu():
    from gpe_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_double * 64)()                      # host memory stands in for the pointers that are checked, never followed
    p = ctypes.addressof(buf)
    st = dict(tags=p, t_sb=8, t_sp=8, t_sl=8, D=3, logit=p, m_sb=8, m_sp=8, m_sl=8, stitches=p, nums=p, S=24, gt_mask=p, gt_tags=p,
              B=2, P=2, L=4, flags=15, margin=0.3, sup_w=0.1, part=p)
    fwd = lambda **kw: l.gpe_stitch_loss_fwd(*_swap(st, **kw), p, None)
    bwd = lambda g_tags=p, g_mask=p, **kw: l.gpe_stitch_loss_bwd(*_swap(st, **kw), None, g_tags, g_mask, None)
    for bad in (dict(S=65), dict(S=65, flags=1), dict(D=9), dict(D=9, flags=8), dict(D=9, flags=1), dict(part=None), dict(part=None, flags=0),
                dict(S=0), dict(D=0), dict(B=0), dict(tags=None), dict(gt_tags=None), dict(gt_mask=None), dict(logit=None), dict(nums=None)):
        assert fwd(**bad) == -22, bad
        assert bwd(**bad) == -22, bad
    assert l.gpe_stitch_loss_fwd(*_swap(st), None, None) == -22                      # out5 NULL
    for flags in (1, 3, 8, 9, 15):
        assert bwd(g_tags=None, flags=flags) == -22, flags                             # g_tags missing under bits 1 | 8
    for flags in (4, 5, 12, 15):
        assert bwd(g_mask=None, flags=flags) == -22, flags                             # g_mask missing under bit 4
    pt = dict(ol=p, ol_sb=8, ol_sp=8, ol_sl=8, rot=p, rot_s=7, tr=p, tr_s=7, gt_ol=p, gt_rot=p, gt_tr=p, num_edges=p, B=2, P=2, L=4, R=4,
              T=3, flags=15, pad0=0.0, pad1=0.0, loop_w=1.0)
    pf = lambda part=p, loop_sums=p, out5=p, **kw: l.gpe_pattern_loss_fwd(*_swap(pt, **kw), part, loop_sums, out5, None)
    pb = lambda loop_sums=p, g_ol=p, **kw: l.gpe_pattern_loss_bwd(*_swap(pt, **kw), loop_sums, None, g_ol, None, None, None)
    for bad in (dict(flags=16), dict(flags=31), dict(flags=-1), dict(B=0), dict(P=0), dict(L=0), dict(ol=None), dict(gt_ol=None, flags=2),
                dict(num_edges=None), dict(rot=None), dict(gt_tr=None), dict(R=0), dict(T=0)):
        assert pf(**bad) == -22, bad
        assert pb(**bad) == -22, bad
    assert pf(part=None) == -22 and pf(out5=None) == -22 and pf(loop_sums=None) == -22
    assert pb(g_ol=None) == -22 and pb(loop_sums=None) == -22
    rn = lambda stitches=p, nums=p, B=2, S=70, P=2, L=4, perm=p, lead=p, num_edges=p, out=p: l.gpe_stitch_renumber(
        stitches, nums, B, S, P, L, perm, lead, num_edges, out, None)
    assert rn(num_edges=None) == -22                                                 # lead without num_edges
    for bad in (dict(stitches=None), dict(nums=None), dict(out=None), dict(B=0), dict(S=0), dict(P=0), dict(L=0)):
        assert rn(**bad) == -22, bad
    ps = lambda feat=p, D=1, lead=p, num_edges=p, npanels=4, L=4, out=p: l.gpe_panel_shift(feat, D, lead, num_edges, npanels, L, out, None)
    for bad in (dict(feat=None), dict(lead=None), dict(num_edges=None), dict(out=None), dict(D=0), dict(npanels=0), dict(L=0)):
        assert ps(**bad) == -22, bad
