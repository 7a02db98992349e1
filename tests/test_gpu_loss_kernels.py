"""-m gpu: the pattern and stitch loss kernels, the stitch renumbering and the panel shift, one by one through the C ABI against the
fp64 references of tests/loss_restate.py (cases, references, the checker and its bars are there, with the table branch -> case;
tests/test_loss_host.py checks them on the CPU first).  No case is filtered.

Every out5 slot is held to 2e-6 max(1, |ref|) and every gradient tensor to relerr < 2e-6 (g_tags / g_mask and g_ol / g_rot / g_tr
each on their own), exactly 0 wherever the reference is exactly 0; a NaN (a pattern without stitches) must be a NaN in the same
slot on both sides; the renumbering and the shift are exact.  Predictions are views into larger tensors whose other elements are
NaN, outputs are longer than their extent and pre-filled with a sentinel, and every call runs twice on fresh buffers: the two
results are the same bits.  The backward kernels run against the `part` / `loop_sums` their forward left behind.

Worst figures observed on an MI355X are in each test's docstring, as relerr or in units of the 2e-6 bar."""
import numpy as np
import pytest
import torch

import loss_restate as R

pytestmark = pytest.mark.gpu

FWD_OF = {'stitch_loss_bwd': 'stitch_loss_fwd', 'pattern_loss_bwd': 'pattern_loss_fwd'}
WORST = {}


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _device(case, kernels):
    host = dict(case.inp)
    for k in kernels:
        host.update(case.out0[k])
    return {n: torch.from_numpy(a.copy()).cuda() for n, a in host.items()}


def _run(gpe, case, kernel):
    """-> {kernel: {name: whole output buffer}} for the entry point and, for a backward, the forward run in front of it"""
    chain = ([FWD_OF[kernel]] if kernel in FWD_OF else []) + [kernel]
    dev = _device(case, chain)
    for k in chain:
        gpe._lib.call('gpe_' + k, *R.abi_args(case, k, dev))
    torch.cuda.synchronize()
    return {k: {n: dev[n].cpu().numpy() for n in case.out0[k]} for k in chain}


def _check(gpe, kernel, case):
    got = _run(gpe, case, kernel)
    again = _run(gpe, case, kernel)
    for k in got:
        for n in got[k]:
            assert got[k][n].tobytes() == again[k][n].tobytes(), '%s[%s] %s: two runs differ' % (k, case.id, n)
    worst = R.check(case, kernel, got[kernel])
    if kernel in FWD_OF:                    # the workspace the backward read is the one the forward checker accepts
        R.check(case, FWD_OF[kernel], got[FWD_OF[kernel]])
    for n, v in worst.items():
        WORST[(kernel, n)] = max(WORST.get((kernel, n), 0.0), v)
    print('%s[%s] worst, in bars of 2e-6: %s' % (kernel, case.id, ', '.join('%s %.4f' % kv for kv in sorted(worst.items())) or 'exact'))


def _cases(kernel):
    return pytest.mark.parametrize('case', R.cases(kernel), ids=R.case_ids(kernel))


@_cases('stitch_loss_fwd')
def test_stitch_loss_fwd(gpe, case):
    """out5 = {total, similarity, negative, supervised, free}; part[b][2] == 2 n_b and part[b][0] the per-pattern similarity (NaN
    for n_b = 0).  MI355X: worst 0.020 bars (total), 0.010 (similarity), 0.006 (negative), 0.007 (supervised), 0.019 (free),
    0.007 (part)."""
    _check(gpe, 'stitch_loss_fwd', case)


@_cases('stitch_loss_bwd')
def test_stitch_loss_bwd(gpe, case):
    """g_tags and g_mask, each by relerr, zeros exact, against the forward's own part.
    MI355X: worst relerr 1.3e-7 = 0.063 bars (g_tags), 8.6e-8 = 0.043 (g_mask)."""
    _check(gpe, 'stitch_loss_bwd', case)


@_cases('pattern_loss_fwd')
def test_pattern_loss_fwd(gpe, case):
    """out5 = {total, shape, loop, rotation, translation}; loop_sums untouched without bit 2.
    MI355X: worst 0.057 bars (total, loop), 0.043 (shape), 0.031 (rotation), 0.030 (translation)."""
    _check(gpe, 'pattern_loss_fwd', case)


@_cases('pattern_loss_bwd')
def test_pattern_loss_bwd(gpe, case):
    """g_ol, g_rot, g_tr, each by relerr; columns 2-3 of the loop term, padding edges and short panels exactly 0.
    MI355X: worst relerr 2.0e-7 = 0.10 bars (g_ol), 1.1e-7 = 0.055 (g_rot), 1.4e-7 = 0.069 (g_tr)."""
    _check(gpe, 'pattern_loss_bwd', case)


@_cases('stitch_renumber')
def test_stitch_renumber(gpe, case):
    """integers, exact, against the oracle's _stitch_after_permute and _gt_stitches_shift; entries past nums[b] copied.  MI355X: exact."""
    _check(gpe, 'stitch_renumber', case)


@_cases('panel_shift')
def test_panel_shift(gpe, case):
    """copies, exact, against the oracle's _per_panel_shift.  MI355X: exact."""
    _check(gpe, 'panel_shift', case)


def test_worst_figures():
    """prints the largest error of every output over the cases that ran (relerr or value error, in units of the 2e-6 bar)"""
    for (kernel, name), v in sorted(WORST.items()):
        print('WORST %-18s %-9s %.4f bars = %.2e' % (kernel, name, v, v * 2e-6))
        assert v < 1.0


# ----------------------------------------------------------------------------------------------------------------------
# the Python wrappers: argument order and which gradients are asked for
# ----------------------------------------------------------------------------------------------------------------------
def _pick(kernel, head):
    return next(c for c in R.cases(kernel) if c.id.startswith(head))


def _rel(got, ref):
    return R.relerr(got.detach().cpu().double().numpy().reshape(-1), np.asarray(ref).reshape(-1))


@pytest.mark.parametrize('head', ['3-2-4-3-3-f15-', '3-2-4-3-3-f8-', '3-2-4-3-3-f4-'])
def test_stitch_loss_wrapper(gpe, head):
    """ops.StitchLossFn on the second shape: the five values, the gradients on the views' columns of the decoder output and zeros
    on every other column; with bit 4 off no g_mask is computed, with bits 1 | 8 off no g_tags"""
    case = _pick('stitch_loss_fwd', head)
    p, ref = case.p, R.expected(case)
    dev = {n: torch.from_numpy(a.copy()).cuda() for n, a in case.inp.items()}
    base = {b: dev[b].requires_grad_() for b in {case.view[n][0] for n in ('tags', 'logit')}}
    view = lambda n: base[case.view[n][0]][case.view[n][1]]
    out = gpe.ops.StitchLossFn.apply(view('tags'), view('logit'), dev['stitches'], dev['nums'], dev['gt_mask'], dev['gt_tags'], p['flags'],
                                     p['margin'], p['sup_w'])
    gs = 1.0 if p['gscale'] is None else p['gscale']
    (out[0] * gs).backward()
    R.check(case, 'stitch_loss_fwd', {'out5': np.concatenate([out.detach().cpu().numpy(), case.out0['stitch_loss_fwd']['out5'][5:]]),
                                      'part': R.emulate(case, 'stitch_loss_fwd')['part']})
    grads = {b: (t.grad if t.grad is not None else torch.zeros_like(t)) for b, t in base.items()}
    for n, key in (('tags', 'g_tags'), ('logit', 'g_mask')):
        g = grads[case.view[n][0]][case.view[n][1]]
        if np.abs(ref[key]).max() == 0:
            assert (g == 0).all(), key
        else:
            assert _rel(g, ref[key]) < 2e-6, (key, _rel(g, ref[key]))
        g.zero_()
    assert all((g == 0).all() for g in grads.values())         # nothing landed outside the two views


@pytest.mark.parametrize('rot_grad', [True, False])
def test_pattern_loss_wrapper(gpe, rot_grad):
    """ops.PatternLossFn on the second shape with all four terms; g_rot is computed only when the rotations require grad"""
    case = _pick('pattern_loss_fwd', '3-2-4-1-5-f15-')
    p, ref = case.p, R.expected(case)
    B, P = p['B'], p['P']
    dev = {n: torch.from_numpy(a.copy()).cuda() for n, a in case.inp.items()}
    panels, place = dev[case.view['ol'][0]].requires_grad_(), dev[case.view['rot'][0]].requires_grad_()
    ol = panels[case.view['ol'][1]]
    rows = lambda n: place.view(B, P, -1)[:, :, case.view[n][1][1]]
    rot = rows('rot') if rot_grad else rows('rot').detach()
    out = gpe.ops.PatternLossFn.apply(ol, rot, rows('tr'), dev['gt_ol'], dev['gt_rot'], dev['gt_tr'], dev['num_edges'], p['flags'],
                                      p['pad'][0], p['pad'][1], p['loop_w'])
    gs = 1.0 if p['gscale'] is None else p['gscale']
    (out[0] * gs).backward()
    R.check(case, 'pattern_loss_fwd', {**R.emulate(case, 'pattern_loss_fwd'),
                                       'out5': np.concatenate([out.detach().cpu().numpy(), case.out0['pattern_loss_fwd']['out5'][5:]])})
    assert _rel(panels.grad[case.view['ol'][1]], ref['g_ol']) < 2e-6
    g = place.grad.view(B, P, -1)
    assert _rel(g[:, :, case.view['tr'][1][1]], ref['g_tr']) < 2e-6
    if rot_grad:
        assert _rel(g[:, :, case.view['rot'][1][1]], ref['g_rot']) < 2e-6
    else:
        assert (g[:, :, case.view['rot'][1][1]] == 0).all()


def test_renumber_and_shift_wrappers(gpe):
    """ops.stitch_renumber (both steps, a repeated perm entry) and ops.panel_shift ([B,P,L,D] and the 3-d mask) on the second shapes"""
    case = _pick('stitch_renumber', '3-5-4-5-rep-lead')
    p = case.p
    dev = {n: torch.from_numpy(a.copy()).cuda() for n, a in case.inp.items()}
    out = gpe.ops.stitch_renumber(dev['stitches'], dev['nums'], p['P'], p['L'], perm=dev['perm'], lead=dev['lead'], num_edges=dev['num_edges'])
    assert np.array_equal(out.cpu().numpy(), R.expected(case)['out'])
    for head in ('7-3-3', '7-3-1'):
        case = _pick('panel_shift', head)
        dev = {n: torch.from_numpy(a.copy()).cuda() for n, a in case.inp.items()}
        feat = dev['feat'][None] if head == '7-3-3' else dev['feat'][None, :, :, 0]
        out = gpe.ops.panel_shift(feat, dev['lead'], dev['num_edges'])
        assert out.shape == feat.shape and np.array_equal(out.cpu().numpy().reshape(-1), R.expected(case)['out'].reshape(-1))
