"""-m gpu: the quality metrics of ComposedPatternLoss on the device (csrc/gpe_quality.hip through ops.quality_metrics) against
  (1) the reference's own numbers (tests/golden/quality_*.pt, scripts/make_quality_golden.py),
  (2) the fp64 restatement of the definitions (tests/quality_restate.py) on randomised garment-shaped batches,
plus the gate (no quality work in grad-enabled calls by default, a refusal inside a stream capture), the documented tie rule of
the greedy stitch pairing, the sigmoid-round decision, run-to-run reproducibility and an end-to-end evaluation pass."""
import copy
import glob
import math
import os

import numpy as np
import pytest
import torch

import quality_restate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, 'golden', 'quality_*.pt')))
EXACT = ('num_panels_accuracy', 'num_edges_accuracy', 'corr_num_edges_accuracy', 'stitch_precision', 'stitch_recall',
         'corr_stitch_precision', 'corr_stitch_recall', 'free_edge_acc')


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _cuda(d):
    return {k: v.clone().cuda() for k, v in d.items()}


def _loss(gpe, dc, lc):
    return gpe.metrics.ComposedPatternLoss(copy.deepcopy(dc), copy.deepcopy(lc))


def _qkeys(gpe):
    return set(gpe.ops.QUALITY_KEYS)


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[8:-3] for f in FIXTURES])
def test_fixture_on_device(gpe, path):
    fx = torch.load(path, weights_only=False)
    loss = _loss(gpe, fx['data_config'], fx['loss_config'])
    with torch.no_grad():
        _, d, _ = loss(_cuda(fx['preds']), _cuda(fx['gt']), epoch=fx['epoch'])
    ref = fx['loss_dict']
    assert set(d) == set(ref)
    q = _qkeys(gpe) & set(ref)
    assert q, 'the fixture has quality keys'
    for k in q:
        v, r = d[k], ref[k]
        if r is None:
            assert v is None, k
            continue
        assert torch.is_tensor(v) and v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda, k
        got = float(v)
        if math.isnan(r):
            assert math.isnan(got), k
        elif k in EXACT:
            assert np.float32(got) == np.float32(r), (k, got, r)
        else:
            assert got == pytest.approx(r, rel=1e-5), (k, got, r)


RANDOM_CASES = [(1, 11, False), (17, 12, False), (64, 13, False), (40, 14, True)]


@pytest.mark.parametrize('B,seed,explicit', RANDOM_CASES)
def test_random_batches_against_restatement(gpe, B, seed, explicit):
    fx = torch.load(os.path.join(HERE, 'golden', 'quality_lstm_e40.pt'), weights_only=False)
    dc, lc = copy.deepcopy(fx['data_config']), fx['loss_config']
    dc['explicit_stitch_tags'] = explicit
    P, L, S = dc['max_pattern_len'], dc['max_panel_len'], dc['max_num_stitches']
    rng = np.random.default_rng(seed)
    kinds = ['ok', 'pad_real', 'open', 'extra', 'odd', 'free0', 'free1', 'nost', 'ok', 'ok']
    for _ in range(100):                                   # re-draw until every decision has its margin
        preds, gt = quality_restate.make_batch(rng, B, P, L, S, dc, kinds[seed % 3:], all_stitches=B == 64)
        want, margin = quality_restate.restate(lc['quality_components'], 40, lc['epoch_with_stitches'], dc['standardize'],
                                               explicit, preds, gt)
        if margin >= quality_restate.MARGIN:
            break
    else:
        pytest.fail('no draw with the decision margin')
    loss = _loss(gpe, dc, lc)
    with torch.no_grad():
        _, d, _ = loss(_cuda(preds), _cuda(gt), epoch=40)
    for k, w in want.items():
        if w is None:
            assert d[k] is None, k
        elif math.isnan(w):
            assert math.isnan(float(d[k])), k
        else:
            assert float(d[k]) == pytest.approx(w, rel=1e-5, abs=1e-7), (k, float(d[k]), w)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _grad_run(gpe, fx, **attrs):
    loss = _loss(gpe, fx['data_config'], fx['loss_config'])
    for k, v in attrs.items():
        setattr(loss, k, v)
    preds = {k: v.clone().cuda().requires_grad_(v.is_floating_point()) for k, v in fx['preds'].items()}
    total, d, _ = loss(preds, _cuda(fx['gt']), epoch=fx['epoch'])
    total.backward()
    torch.cuda.synchronize()
    return total.detach(), {k: v.grad for k, v in preds.items() if v.grad is not None}, d


def test_gate(gpe):
    fx = torch.load(os.path.join(HERE, 'golden', 'quality_lstm_e40.pt'), weights_only=False)
    qk = _qkeys(gpe)
    l0, g0, d0 = _grad_run(gpe, fx, with_quality_eval=False)
    l1, g1, d1 = _grad_run(gpe, fx)                          # defaults: with_quality_eval on, autograd recording
    assert not (set(d1) & qk) and set(d1) == set(d0)
    assert _same_bits(l0, l1) and set(g0) == set(g1) and all(_same_bits(g0[k], g1[k]) for k in g0)
    l2, g2, d2 = _grad_run(gpe, fx, quality_in_training=True)
    assert set(d2) & qk == qk & set(fx['loss_dict'])
    assert _same_bits(l0, l2) and all(_same_bits(g0[k], g2[k]) for k in g0)
    loss = _loss(gpe, fx['data_config'], fx['loss_config'])
    with torch.no_grad():
        _, d3, _ = loss(_cuda(fx['preds']), _cuda(fx['gt']), epoch=fx['epoch'])
    assert set(d3) & qk == qk & set(fx['loss_dict'])
    for k in qk & set(d3):
        if d3[k] is not None:
            assert _same_bits(d3[k], d2[k]), k


def test_capture_refuses_quality(gpe):
    fx = torch.load(os.path.join(HERE, 'golden', 'quality_lstm_e0.pt'), weights_only=False)
    loss = _loss(gpe, fx['data_config'], fx['loss_config'])
    preds, gt = _cuda(fx['preds']), _cuda(fx['gt'])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        loss.with_quality_eval = False
        loss(preds, dict(gt), epoch=0)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    loss.with_quality_eval = True
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='stream capture'):
        with torch.no_grad(), torch.cuda.graph(g):
            loss(preds, dict(gt), epoch=0)
    torch.cuda.synchronize()


def _stitch_case(gpe, tags_pts, gt_pairs, P=4, L=4):
    """one pattern whose non-free edges are 0 .. len(tags_pts)-1 (edge order) with the given 3-D tags"""
    fx = torch.load(os.path.join(HERE, 'golden', 'quality_lstm_e40.pt'), weights_only=False)
    dc, lc = copy.deepcopy(fx['data_config']), copy.deepcopy(fx['loss_config'])
    lc['quality_components'] = ['stitch']
    dc['max_pattern_len'], dc['max_panel_len'] = P, L
    m = len(tags_pts)
    tags = torch.zeros(1, P, L, 3)
    tags.view(-1, 3)[:m] = torch.tensor(tags_pts, dtype=torch.float32)
    logit = torch.full((1, P, L), 3.0)
    logit.view(-1)[:m] = -3.0
    S = 24
    st = torch.zeros(1, 2, S, dtype=torch.long)
    for k, (a, b) in enumerate(gt_pairs):
        st[0, 0, k], st[0, 1, k] = a, b
    preds = {'outlines': torch.zeros(1, P, L, 4), 'rotations': torch.zeros(1, P, 4), 'translations': torch.zeros(1, P, 3),
             'stitch_tags': tags, 'free_edges_mask': logit}
    gt = {'outlines': torch.zeros(1, P, L, 4), 'num_edges': torch.full((1, P), 4), 'num_panels': torch.tensor([P]),
          'rotations': torch.zeros(1, P, 4), 'translations': torch.zeros(1, P, 3), 'stitches': st,
          'num_stitches': torch.tensor([len(gt_pairs)]), 'free_edges_mask': logit > 0}
    loss = _loss(gpe, dc, lc)
    with torch.no_grad():
        _, d, _ = loss(_cuda(preds), _cuda(gt), epoch=40)
    return float(d['stitch_precision']), float(d['stitch_recall'])


def test_stitch_pairing_tie_rule(gpe):
    # unit square: d(0,1) = d(0,2) = d(1,3) = d(2,3) = 1 exactly; the row-major first minimum is (0, 1), then (2, 3)
    sq = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]
    assert _stitch_case(gpe, sq, [(0, 1), (2, 3)]) == (1.0, 1.0)
    assert _stitch_case(gpe, sq, [(0, 2), (1, 3)]) == (0.0, 0.0)
    # eight points on a line with unit spacing: (0,1), (2,3), (4,5), (6,7) — every step a tie with its neighbours
    line = [(float(i), 0, 0) for i in range(8)]
    assert _stitch_case(gpe, line, [(0, 1), (2, 3), (4, 5), (6, 7)]) == (1.0, 1.0)
    margins = []
    assert sorted(quality_restate.greedy_pairs(np.array(line), margins)) == [(0, 1), (2, 3), (4, 5), (6, 7)]


def test_sigmoid_round_decision_matches_torch(gpe):
    fx = torch.load(os.path.join(HERE, 'golden', 'quality_lstm_e40.pt'), weights_only=False)
    dc, lc = copy.deepcopy(fx['data_config']), copy.deepcopy(fx['loss_config'])
    lc['quality_components'] = ['free_class']
    B, P, L = 64, dc['max_pattern_len'], dc['max_panel_len']
    n = B * P * L
    for step in (2.0 ** -26, 2.0 ** -30, 2.0 ** -12):
        k = torch.arange(n, dtype=torch.float64) - n // 2
        x = (k * step).float().cuda().view(B, P, L)
        gt_mask = torch.round(torch.sigmoid(x))                 # torch's decision on the same device
        assert 0 < int(gt_mask.sum()) < n
        preds = {'outlines': torch.zeros(B, P, L, 4, device='cuda'), 'free_edges_mask': x,
                 'rotations': torch.zeros(B, P, 4, device='cuda'), 'translations': torch.zeros(B, P, 3, device='cuda'),
                 'stitch_tags': torch.zeros(B, P, L, 3, device='cuda')}
        gt = {'outlines': torch.zeros(B, P, L, 4, device='cuda'), 'num_edges': torch.zeros(B, P, device='cuda', dtype=torch.long),
              'rotations': torch.zeros(B, P, 4, device='cuda'), 'translations': torch.zeros(B, P, 3, device='cuda'),
              'free_edges_mask': gt_mask.bool(), 'stitches': torch.zeros(B, 2, 24, dtype=torch.long, device='cuda'),
              'num_stitches': torch.zeros(B, dtype=torch.long, device='cuda')}
        loss = _loss(gpe, dc, lc)
        with torch.no_grad():
            _, d, _ = loss(preds, gt, epoch=40)
        assert float(d['free_edge_acc']) == 1.0, step


def test_two_calls_bit_identical(gpe):
    fx = torch.load(os.path.join(HERE, 'golden', 'quality_full.pt'), weights_only=False)
    loss = _loss(gpe, fx['data_config'], fx['loss_config'])
    vecs = []
    for _ in range(2):
        with torch.no_grad():
            loss(_cuda(fx['preds']), _cuda(fx['gt']), epoch=fx['epoch'])
        vecs.append(loss.last_quality_vector.clone())
    assert _same_bits(vecs[0], vecs[1])


def test_end_to_end_eval_pass(gpe):
    fx = torch.load(os.path.join(HERE, 'golden', 'full3d_shipped.pt'), weights_only=False)
    q = torch.load(os.path.join(HERE, 'golden', 'quality_lstm_e40.pt'), weights_only=False)
    torch.manual_seed(0)
    model = gpe.nets.GarmentFullPattern3D(fx['data_config'], copy.deepcopy(fx['nn_config']),
                                          copy.deepcopy(q['loss_config'])).cuda().eval()
    B = 8
    feats = torch.randn(B, fx['N'], 3, device='cuda')
    gt = {k: v[:B].cuda() for k, v in q['gt'].items()}
    with torch.no_grad():
        preds = model(feats)
        _, d, _ = model.loss(preds, gt, epoch=40)
    qk = _qkeys(gpe) & set(d)
    assert qk == set(k for k in q['loss_dict'] if k in _qkeys(gpe))
    none_correct = float(d['num_panels_accuracy']) == 0.0
    for k in qk:
        if k.startswith('corr_') and none_correct:               # no pattern with the right panel count: None / NaN by definition
            assert d[k] is None or math.isnan(float(d[k])), k
            continue
        assert d[k] is not None and math.isfinite(float(d[k])), k
