"""-m gpu: the edge-pair classifier scored over all edge pairs against ground-truth stitches on the device
(csrc/gpe_stitch_pairs.hip's evaluating instantiations through ops.stitch_pairs_eval / StitchOnEdge3DPairs.evaluate_stitches)
against the fp64 restatement (tests/stitch_eval_restate.py), which tests/test_stitch_eval_host.py pins to the reference's recorded
numbers.  Every test runs both routes in every arithmetic mode with the f16x3 size gate lifted, on the garments of
tests/golden/stitch_pairs_*.pt with their planted stitches as ground truth (each plant in its own orientation).

Bars.  Every logit of the shipped-weights fixtures is >= 4 tol away from 0 (tol = 1e-4 * max(1, max |logit|), the project's logit
bar), so the class of every pair and with it every counter is exact in every arithmetic.  A BCE-with-logits term is 1-Lipschitz in
the logit, so the mean loss moves by less than tol; the device evaluates a term as the sum of two non-negative fp32 numbers from
expf / log1pf (a few ulp of 2^-24 each) and adds in fp64, which is within 2^-20 relative of the exact term of the same logit."""
import functools
import os

import numpy as np
import pytest
import torch

import stitch_pairs_restate as R
import stitch_eval_restate as EV
import test_gpu_stitch_pairs as SP          # the garments, models and padding of the prediction tests (helpers only)

pytestmark = pytest.mark.gpu

FIXTURES, IDS, ROUTES = SP.FIXTURES, SP.IDS, SP.ROUTES
COUNTS = EV.COUNTS
REL = 2.0 ** -20


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


@pytest.fixture(scope='module')
def known():
    return torch.load(os.path.join(SP.HERE, 'golden', 'stitch_pairs_known_answer.pt'), weights_only=False)


@functools.lru_cache(maxsize=None)
def _fixture(path):
    fx = SP._load(path)
    fx['gt'] = [(tuple(a), tuple(b)) for a, b in fx['plants']]
    return fx


@functools.lru_cache(maxsize=None)
def _shipped_reference(path):
    """computed once per garment: fp64 logits of the shipped weights and their evaluation"""
    fx = _fixture(path)
    known = torch.load(os.path.join(SP.HERE, 'golden', 'stitch_pairs_known_answer.pt'), weights_only=False)
    lg64 = SP._lg64(known['state_dict'], fx)
    return lg64, EV.evaluate(fx['pairs'], lg64, fx['gt'])


def _ids(stitches, L, S=None):
    """ground truth in the product's layout: int64 [2, S] of edge ids panel * L + edge, zero-padded, and the count"""
    S = len(stitches) if S is None else S
    t = torch.zeros(2, S, dtype=torch.int64)
    for n, (a, b) in enumerate(stitches):
        t[0, n], t[1, n] = a[0] * L + a[1], b[0] * L + b[1]
    return t, len(stitches)


def _evaluate(model, edges, ne, gt, n, stats, route, logits=False):
    out, loss_dict = model.evaluate_stitches(edges.cuda(), ne.cuda(), gt.cuda(), n.cuda(), stats, route=route, return_logits=logits)
    assert all(v.is_cuda for k, v in out.items() if k != 'metrics') and all(v.is_cuda for v in out['metrics'].values())
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in loss_dict.values())
    assert set(loss_dict) == {'edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall'}
    for k, v in loss_dict.items():
        assert torch.equal(v, out['metrics'][k])
    assert out['counts'].dtype == torch.int32 and out['loss_sum'].dtype == torch.float64
    cpu = {k: v.cpu() for k, v in out.items() if k != 'metrics'}
    cpu['metrics'] = {k: v.cpu().numpy()[()] for k, v in out['metrics'].items()}
    return cpu


def _one(model, fx, route, logits=False, gt=None, n=None):
    L = fx['edges'].shape[1]
    if gt is None:
        gt, n = _ids(fx['gt'], L)
    return _evaluate(model, fx['edges'][None], fx['num_edges'][None], gt[None], torch.tensor([n]), fx['stats'], route, logits)


def _f32_ratio(num, den):
    return np.float32(num) / np.float32(den) if den else np.float32(0)


def _check_counts_and_ratios(out, b, want, single_call):
    got = dict(zip(COUNTS, out['counts'][b].tolist()))
    assert got == {k: want['counts'][k] for k in COUNTS}, (got, want['counts'])
    assert int(out['num_stitches'][b]) == want['counts']['selected']
    if single_call:
        c, m = want['counts'], out['metrics']
        assert m['edge_pair_class_acc'] == _f32_ratio(c['correct'], c['pairs'])
        assert m['stitch_precision'] == _f32_ratio(c['true_positives'], c['predicted_positives'])
        assert m['stitch_recall'] == _f32_ratio(c['true_positives'], c['gt_positives'])
        assert m['selected_precision'] == _f32_ratio(c['selected_tp'], c['selected'])
        assert m['selected_recall'] == _f32_ratio(c['selected_tp'], c['gt_positives'])
        mean = float(out['loss_sum'][b]) / c['pairs'] if c['pairs'] else 0.0
        assert m['edge_pair_class_loss'] == np.float32(mean)


def _check_own_logits(out, b, fx, L):
    """the epilogue and the reductions, whatever the arithmetic: fp64 BCE and the counters of the product's OWN fp32 logits"""
    own = R.dense_to_list(out['logits'][b].numpy(), fx['pairs'], L) if fx['pairs'] else np.zeros(0, dtype=np.float32)
    want = EV.evaluate(fx['pairs'], own, fx['gt'])
    got, ref = float(out['loss_sum'][b]), want['loss_sum']
    print('garment %s: loss_sum %.12g, fp64 of its own logits %.12g, relative %.3g (bar 2^-20 = %.3g)'
          % (fx['tag'], got, ref, abs(got - ref) / ref if ref else 0.0, REL))
    assert abs(got - ref) <= REL * ref
    return want


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_fixture_against_fp64_logits(gpe, known, math_mode, path, route):
    fx = _fixture(path)
    lg64, want = _shipped_reference(path)
    out = _one(SP._shipped(gpe, known), fx, route)
    assert set(out) == {'stitches', 'num_stitches', 'scores', 'metrics', 'counts', 'loss_sum'}
    _check_counts_and_ratios(out, 0, want, True)
    loss64 = want['loss_sum'] / len(fx['pairs'])
    loss = float(out['loss_sum'][0]) / len(fx['pairs'])
    bar = fx['tol'] + REL * max(1.0, loss64)
    print('garment %s: loss %.9g, fp64 %.9g, |difference| %.3g (bar %.3g)' % (fx['tag'], loss, loss64, abs(loss - loss64), bar))
    assert abs(loss - loss64) < bar
    assert abs(float(out['metrics']['edge_pair_class_loss']) - loss64) < bar


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_fixture_against_its_own_logits(gpe, known, math_mode, path, route):
    fx = _fixture(path)
    out = _one(SP._shipped(gpe, known), fx, route, logits=True)
    want = _check_own_logits(out, 0, fx, fx['edges'].shape[1])
    _check_counts_and_ratios(out, 0, want, True)
    assert want['counts'] == _shipped_reference(path)[1]['counts']          # the margins make the classes those of the fp64 logits


@pytest.mark.parametrize('hidden,layers,routes', [(64, 1, ROUTES), (200, 3, ROUTES), (30, 5, ('auto',))])
def test_random_weights(gpe, math_mode, hidden, layers, routes):
    """two accumulator widths of the fused kernel (4 and 13 column blocks) and one shape off its menu; counters from the product's
    own logits only: random weights carry no decision margins"""
    model = SP._random_model(gpe, hidden, layers, 100 + hidden)
    assert gpe.ops.stitch_pairs_on_menu(model.mlp) == (routes != ('auto',))
    fx = _fixture([f for f in FIXTURES if f.endswith('gaps.pt')][0])
    for route in routes:
        out = _one(model, fx, route, logits=True)
        want = _check_own_logits(out, 0, fx, fx['edges'].shape[1])
        _check_counts_and_ratios(out, 0, want, True)
        assert 0 < want['counts']['predicted_positives'] < want['counts']['pairs']


@pytest.mark.parametrize('route', ROUTES)
def test_batched_equals_per_garment_and_repeats_bit_identically(gpe, known, math_mode, route):
    fxs = [_fixture(f) for f in FIXTURES]
    model = SP._shipped(gpe, known)
    P = max(fx['edges'].shape[0] for fx in fxs) + 1
    L = max(fx['edges'].shape[1] for fx in fxs) + 2
    padded = [SP._padded(fx, P, L) for fx in fxs]
    edges, ne = torch.stack([p[0] for p in padded]), torch.stack([p[1] for p in padded])
    S = max(len(fx['gt']) for fx in fxs) + 3
    gts = [_ids(fx['gt'], L, S) for fx in fxs]
    gt, n = torch.stack([g[0] for g in gts]), torch.tensor([g[1] for g in gts])
    for g, k in zip(gt, n):
        g[:, int(k):] = 10 ** 6                                  # whatever lies beyond the count is not read
    stats = fxs[0]['stats']
    a = _evaluate(model, edges, ne, gt, n, stats, route)
    b = _evaluate(model, edges, ne, gt, n, stats, route)
    for k in ('stitches', 'num_stitches', 'scores', 'counts', 'loss_sum'):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert all(a['metrics'][k].tobytes() == b['metrics'][k].tobytes() for k in a['metrics'])
    total, pairs = 0.0, 0
    for i, fx in enumerate(fxs):
        want = _shipped_reference(FIXTURES[i])[1]
        _check_counts_and_ratios(a, i, want, False)
        one = _evaluate(model, edges[i:i + 1], ne[i:i + 1], gt[i:i + 1], n[i:i + 1], stats, route)
        assert torch.equal(one['counts'][0], a['counts'][i]), fx['tag']
        assert torch.equal(one['loss_sum'][0].view(torch.int64), a['loss_sum'][i].view(torch.int64)), fx['tag']
        total += float(a['loss_sum'][i])                         # in garment order, as the finalisation adds
        pairs += want['counts']['pairs']
    assert a['metrics']['edge_pair_class_loss'] == np.float32(total / pairs)
    pooled = EV.pooled([_shipped_reference(f)[1] for f in FIXTURES])
    for k in ('edge_pair_class_acc', 'stitch_precision', 'stitch_recall', 'selected_precision', 'selected_recall'):
        assert abs(float(a['metrics'][k]) - pooled[k]) <= 2.0 ** -23 * pooled[k], k       # one fp32 division of exact integers


@pytest.mark.parametrize('route', ROUTES)
def test_ground_truth_edge_cases_leave_the_counters_alone(gpe, known, math_mode, route):
    path = [f for f in FIXTURES if f.endswith('small.pt')][0]
    fx = _fixture(path)
    model = SP._shipped(gpe, known)
    P, L = fx['edges'].shape[:2]
    E, ne = P * L, fx['num_edges'].tolist()
    assert ne == [5, 0, 4, 6, 0, 0, 3, 5]
    clean_gt, clean_n = _ids(fx['gt'], L)
    clean = _one(model, fx, route, gt=clean_gt, n=clean_n)
    _check_counts_and_ratios(clean, 0, _shipped_reference(path)[1], True)
    flipped = [(b, a) for a, b in fx['gt']]
    cases = {
        'duplicated': fx['gt'] + fx['gt'][:2],
        'both orientations': fx['gt'] + flipped,
        'flipped only': flipped,
        'ids below 0 and at or above E': fx['gt'] + [((0, -1), (2, 0)), ((0, 0), (P, 0)), ((P + 3, 1), (0, 2)), ((0, -7 * L), (0, 1))],
        'a same-panel pair': fx['gt'] + [((0, 0), (0, 1)), ((3, 2), (3, 2))],
        'an edge beyond num_edges': fx['gt'] + [((0, 5), (2, 0)), ((2, 0), (0, 5)), ((1, 0), (3, 1)), ((6, 3), (7, 4))],
    }
    for name, stitches in cases.items():
        gt, n = _ids(stitches, L)
        assert EV.labels(fx['pairs'], EV.stitches_from_ids(gt.numpy(), n, L)).tolist() == _shipped_reference(path)[1]['mask'].tolist()
        out = _one(model, fx, route, gt=gt, n=n)
        assert torch.equal(out['counts'], clean['counts']), name
        assert torch.equal(out['loss_sum'].view(torch.int64), clean['loss_sum'].view(torch.int64)), name
    # a count larger than S is clamped to S
    out = _one(model, fx, route, gt=clean_gt, n=clean_n + 5)
    assert torch.equal(out['counts'], clean['counts']) and torch.equal(out['loss_sum'], clean['loss_sum'])
    # S = 0 (whatever the count says) and a count of 0: no pair is labelled
    lg64 = _shipped_reference(path)[0]
    empty = EV.evaluate(fx['pairs'], lg64, [])
    for gt, n in ((torch.zeros(2, 0, dtype=torch.int64), 3), (clean_gt, 0), (clean_gt, -2)):
        out = _one(model, fx, route, gt=gt, n=n)
        _check_counts_and_ratios(out, 0, empty, True)
        assert out['counts'][0, 4] == 0 and out['metrics']['stitch_recall'] == 0 and out['metrics']['selected_recall'] == 0


@pytest.mark.parametrize('route', ROUTES)
def test_prediction_outputs_are_those_of_predict_stitches(gpe, known, math_mode, route):
    fxs = [_fixture(f) for f in FIXTURES if not f.endswith('full.pt')]
    model = SP._shipped(gpe, known)
    P, L = max(fx['edges'].shape[0] for fx in fxs), max(fx['edges'].shape[1] for fx in fxs)
    padded = [SP._padded(fx, P, L) for fx in fxs]
    edges, ne = torch.stack([p[0] for p in padded]).cuda(), torch.stack([p[1] for p in padded]).cuda()
    S = max(len(fx['gt']) for fx in fxs)
    gts = [_ids(fx['gt'], L, S) for fx in fxs]
    gt, n = torch.stack([g[0] for g in gts]).int().cuda(), torch.tensor([g[1] for g in gts]).cuda()
    for logits in (False, True):
        pred = model.predict_stitches(edges, ne, fxs[0]['stats'], route=route, return_logits=logits)
        out, loss_dict = model.evaluate_stitches(edges, ne, gt, n, fxs[0]['stats'], route=route, return_logits=logits)
        assert set(out) == set(pred) | {'metrics', 'counts', 'loss_sum'}
        for k, v in pred.items():
            assert out[k].is_cuda and out[k].dtype == v.dtype and torch.equal(out[k].view(torch.int32), v.view(torch.int32)), k
        assert out['counts'].is_cuda and out['loss_sum'].is_cuda and all(v.is_cuda for v in out['metrics'].values())
        assert all(torch.is_tensor(v) and v.is_cuda for v in loss_dict.values())
    with pytest.raises(RuntimeError, match='eval'):
        model.train().evaluate_stitches(edges, ne, gt, n, fxs[0]['stats'])
