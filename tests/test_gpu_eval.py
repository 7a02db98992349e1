"""-m gpu: the evaluation pass on the device (csrc/gpe_eval.hip through ops.EvalAccumulator / ops.quality_pool,
metrics.*.accumulate, evaluation.Evaluator) against
  (1) the numpy restatement of the reference's rule (tests/eval_restate.py) for the accumulator alone,
  (2) that rule applied to what the existing loss.__call__ returns per batch (bit-equal), to the fp64 restatement of the quality
      definitions (tests/quality_restate.py, the bar of test_gpu_quality.py) and to the reference's recorded loss dicts,
  (3) ops.quality_metrics on the concatenated batch / on every group's garments as one batch, for the pooled table (bit-equal),
  (4) the whole path model.predict -> loss, eager and captured, one folder and a dict of folders,
  (5) a MeshPointSampler feeding it, (6) the pair classifier."""
import copy
import glob
import math
import os

import numpy as np
import pytest
import torch

import eval_restate as R
import quality_restate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'quality_*.pt')))
EXACT = ('num_panels_accuracy', 'num_edges_accuracy', 'corr_num_edges_accuracy', 'stitch_precision', 'stitch_recall',
         'corr_stitch_precision', 'corr_stitch_recall', 'free_edge_acc')          # test_gpu_quality.EXACT


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _cuda(d):
    return {k: v.clone().cuda() for k, v in d.items()}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    """bit-equal, a NaN equal to a NaN whatever its payload"""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (a.isnan() & b.isnan())).all())


def _accumulator(gpe, loss, epoch, slots=1):
    keys, gates = loss.eval_keys(epoch)
    return gpe.ops.EvalAccumulator(keys, gates, slots=slots, device='cuda')


# ---- 1. the accumulator alone --------------------------------------------------------------------------------------------------
def test_accumulator_alone(gpe):
    ops = gpe.ops
    lens = (5, 5, 14)
    # 19 keys: 4 of source 0, 4 of source 1, 11 of source 2; three gated ones
    where = [(0, i) for i in range(1, 5)] + [(1, i) for i in range(1, 5)] + [(2, i) for i in range(0, 11)]
    names = ['full_loss'] + ['k%d' % i for i in range(1, 19)]
    keys = [(n, s, i) for n, (s, i) in zip(names, where)]
    at = {w: n for n, w in zip(names, where)}
    assert (at[2, 1], at[2, 2], at[2, 3], at[2, 4]) == ('k9', 'k10', 'k11', 'k12')
    gates = {'k9': 0, 'k10': 1, 'k11': 2}            # k9: counted in adds 1 and 3; k10: never; k11: once (add 2)
    counts = [[0, 0, 0, 9], [1, 0, 0, 9], [0, -1, 4, 9], [7, 0, 0, 9], [0, 0, 0, 9]]
    slot_of = [0, 1, 1, 2, 1]
    rng = np.random.default_rng(5)
    vals = [[rng.normal(0, 3, n).astype(np.float32) for n in lens] for _ in range(5)]
    vals[1][0][2] = np.nan                            # at[0, 2], slot 1
    vals[2][1][3] = np.inf                            # at[1, 3], slot 1
    vals[1][2][4], vals[2][2][4], vals[4][2][4] = np.float32(2e-41), np.float32(1e-41), np.float32(-3.5e-41)      # k12, slot 1: denormals
    vals[3][2][1] = np.float32(-0.0)                  # k9 of slot 2: 0 + -0 = +0, as sum() starts from 0
    acc = ops.EvalAccumulator(keys, gates, slots=3, device='cuda')
    assert acc.slot.dtype == torch.int32 and acc.slot.is_cuda and acc.slot.numel() == 1
    per_slot = [[], [], []]
    for a in range(5):
        acc.set_slot(slot_of[a])
        src = [torch.tensor(v, device='cuda') for v in vals[a]]
        acc.add(*src, counts=torch.tensor(counts[a], dtype=torch.int32, device='cuda'))
        d = {n: R.gate(n, vals[a][s][i], counts[a], gates) for n, s, i in keys[1:]}
        per_slot[slot_of[a]].append((vals[a][0][1], d))
    rows = acc.read()
    assert acc.last_batches.tolist() == [1, 3, 1]
    for s in range(3):
        want_sum, want_cnt = R.sums(per_slot[s])
        for k, n in enumerate(names):
            assert acc.last_counts[s, k] == want_cnt[n], (s, n)
            assert R.same(acc.last_sums[s, k], want_sum[n]), (s, n, acc.last_sums[s, k], want_sum[n])
        R.assert_same(rows[s], R.aggregate(per_slot[s]), 'slot %d' % s)
    assert rows[1]['k10'] is None and rows[0]['k9'] is None and rows[1]['k11'] is not None and acc.last_counts[1, 11] == 1
    assert np.isnan(rows[1][at[0, 2]]) and np.isinf(rows[1][at[1, 3]])
    tiny = np.float32(np.float32(np.float32(2e-41) + np.float32(1e-41)) + np.float32(-3.5e-41))
    assert tiny != 0 and abs(tiny) < 1e-41 and acc.last_sums[1, 12].view(np.int32) == tiny.view(np.int32)         # no flush to zero
    assert acc.last_sums[2, 9].view(np.int32) == 0                                                                # 0 + -0 = +0
    # an out-of-range slot word sets the status and adds nothing
    before = acc.state.clone()
    for bad in (3, -1):
        acc.slot.fill_(bad)
        acc.add(*[torch.ones(n, device='cuda') for n in lens], counts=torch.ones(4, dtype=torch.int32, device='cuda'))
    assert int(acc.status) == 1 and torch.equal(acc.state[:-1], before[:-1])
    with pytest.raises(RuntimeError, match='slot word'):
        acc.read()
    acc.reset()
    assert int(acc.state.abs().sum()) == 0 and int(acc.slot) == 0
    assert all(v is None for v in acc.read()[0].values())


# ---- 2. against the existing loss ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def drawn(gpe):
    """four random garment-shaped batches (17, 17, 5, 1) with the decision margin of test_random_batches_against_restatement; the
    third has no pattern with the right panel count -> [(preds, gt, restated quality dict)], data config, loss config"""
    fx = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    dc, lc = copy.deepcopy(fx['data_config']), fx['loss_config']
    P, L, S = dc['max_pattern_len'], dc['max_panel_len'], dc['max_num_stitches']
    rng = np.random.default_rng(21)
    mixed = ['ok', 'pad_real', 'open', 'extra', 'odd', 'free0', 'free1', 'nost', 'ok', 'ok']
    out = []
    for B, kinds in ((17, mixed), (17, mixed[2:]), (5, ['extra']), (1, ['ok'])):
        for _ in range(100):
            preds, gt = quality_restate.make_batch(rng, B, P, L, S, dc, kinds)
            want, margin = quality_restate.restate(lc['quality_components'], 40, lc['epoch_with_stitches'], dc['standardize'],
                                                   False, preds, gt)
            if margin >= quality_restate.MARGIN:
                break
        else:
            pytest.fail('no draw with the decision margin')
        out.append((preds, gt, want))
    assert out[2][2]['corr_rotation_l2'] is None and out[0][2]['corr_rotation_l2'] is not None
    return out, dc, lc


def test_accumulate_against_the_loss_call(gpe, drawn):
    batches, dc, lc = drawn
    loss = gpe.metrics.ComposedPatternLoss(copy.deepcopy(dc), copy.deepcopy(lc))
    per_batch = []
    with torch.no_grad():
        for preds, gt, _ in batches:
            full, d, _ = loss(_cuda(preds), _cuda(gt), epoch=40)
            per_batch.append((full, d))
    want = R.aggregate(per_batch)
    assert any(d['corr_rotation_l2'] is None for _, d in per_batch) and want['corr_rotation_l2'] is not None
    acc = _accumulator(gpe, loss, 40)
    assert [k[0] for k in acc.keys] == list(want)
    for preds, gt, _ in batches:
        loss.accumulate(_cuda(preds), _cuda(gt), acc, epoch=40)
    got = acc.read()[0]
    for k in want:
        print(k, got[k], want[k])
    R.assert_same(got, want, 'accumulate vs loss.__call__')
    with_corr = sum(w['corr_rotation_l2'] is not None for _, _, w in batches)
    assert acc.last_batches.tolist() == [4] and 2 <= with_corr < 4
    assert acc.last_counts[0, list(want).index('corr_rotation_l2')] == with_corr
    # ... and against the fp64 restatement of the definitions: the bar test_gpu_quality.py holds per batch; the values are
    # non-negative, so their mean inherits it
    ref = R.aggregate([(0.0, w) for _, _, w in batches])
    for k, w in ref.items():
        if k == 'full_loss':
            continue
        if w is None:
            assert got[k] is None, k
        elif math.isnan(w):
            assert math.isnan(got[k]), k
        else:
            assert float(got[k]) == pytest.approx(float(w), rel=1e-5, abs=1e-7), (k, got[k], w)


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[8:-3] for f in FIXTURES])
def test_fixture_as_a_single_batch(gpe, path):
    fx = torch.load(path, weights_only=False)
    loss = gpe.metrics.ComposedPatternLoss(copy.deepcopy(fx['data_config']), copy.deepcopy(fx['loss_config']))
    acc = _accumulator(gpe, loss, fx['epoch'])
    loss.accumulate(_cuda(fx['preds']), _cuda(fx['gt']), acc, epoch=fx['epoch'])
    got = acc.read()[0]
    ref = fx['loss_dict']
    assert set(got) == set(ref) | {'full_loss'}
    with torch.no_grad():
        full, d, _ = loss(_cuda(fx['preds']), _cuda(fx['gt']), epoch=fx['epoch'])
    R.assert_same(got, R.aggregate([(full, d)]), 'one batch: the value itself')
    for k, r in ref.items():                         # the reference's own numbers: the loss terms and the quality metrics
        print(k, got[k], r)
        if r is None:
            assert got[k] is None, k
        elif math.isnan(r):
            assert math.isnan(got[k]), k
        elif k in EXACT:
            assert np.float32(got[k]) == np.float32(r), (k, got[k], r)
        else:
            assert float(got[k]) == pytest.approx(r, rel=1e-5), (k, got[k], r)


def test_accumulate_inside_a_capture_and_call_still_refuses(gpe):
    fx = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    loss = gpe.metrics.ComposedPatternLoss(copy.deepcopy(fx['data_config']), copy.deepcopy(fx['loss_config']))
    preds, gt = _cuda(fx['preds']), _cuda(fx['gt'])
    eager = _accumulator(gpe, loss, 40)
    acc = _accumulator(gpe, loss, 40)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss.accumulate(preds, dict(gt), eager, epoch=40)                 # (also the warm-up)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            loss.accumulate(preds, dict(gt), acc, epoch=40)
        g.replay()
        g.replay()
        side.synchronize()
        g2 = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match='stream capture'):
            with torch.no_grad(), torch.cuda.graph(g2, stream=side):
                loss(preds, dict(gt), epoch=40)
    torch.cuda.synchronize()
    one, two = eager.read()[0], acc.read()[0]
    assert acc.last_batches.tolist() == [2]
    for k, v in one.items():                                              # the same batch twice: 2 v / 2
        assert R.same(two[k], None if v is None else np.float32(np.float32(v + v) / np.float32(2))), k


# ---- 3. pooling ---------------------------------------------------------------------------------------------------------------------
def _quality(loss, preds, gt, part=None):
    """ops.quality_metrics as the loss calls it (the fixture's loss matches nothing: the ground truth is used as it is)"""
    loss.epoch = 40
    return loss._quality_launch(preds, gt, gt['num_edges'].int().view(-1), part)


def _take(d, idx):
    return {k: v[idx].contiguous() for k, v in d.items()}


@pytest.mark.parametrize('sizes', [(17, 17, 5), (64, 64, 5)], ids=['39', '133_crosses_the_fetch'])
def test_pooled_table(gpe, sizes):
    ops = gpe.ops
    fx = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    dc, lc = copy.deepcopy(fx['data_config']), fx['loss_config']
    assert not lc['panel_origin_invariant_loss'] and not lc['panel_order_inariant_loss']
    P, L, S = dc['max_pattern_len'], dc['max_panel_len'], dc['max_num_stitches']
    rng = np.random.default_rng(sum(sizes))
    kinds = ['ok', 'pad_real', 'open', 'extra', 'odd', 'free0', 'free1', 'nost', 'ok', 'ok']
    G = sum(sizes)
    preds, gt = quality_restate.make_batch(rng, G, P, L, S, dc, kinds)
    preds, gt = _cuda(preds), _cuda(gt)
    loss = gpe.metrics.ComposedPatternLoss(dc, copy.deepcopy(lc))
    flags = loss._quality_flags(True)
    table = torch.full((G, 16), float('nan'), device='cuda', dtype=torch.float64)
    g0 = 0
    for B in sizes:
        idx = torch.arange(g0, g0 + B, device='cuda')
        _quality(loss, _take(preds, idx), _take(gt, idx), part=table[g0:g0 + B])
        g0 += B
    want_all = _quality(loss, preds, gt)
    # three interleaved groups, an empty one (3), an id out of range on both sides
    group = (torch.arange(G, dtype=torch.int32) * 7 + 1) % 3
    group[4], group[G - 2] = 9, -1
    group = group.cuda()
    out, counts = ops.quality_pool(table, group, 4, P, L, flags)
    assert out.shape == (5, 14) and counts.shape == (5, 4) and out.dtype == torch.float32 and counts.dtype == torch.int32
    assert _same_bits(out[4], want_all[0]) and torch.equal(counts[4], want_all[1])
    for g in range(3):
        idx = (group == g).nonzero().view(-1)
        assert idx.numel() > 1
        w = _quality(loss, _take(preds, idx), _take(gt, idx))
        assert _same_bits(out[g], w[0]) and torch.equal(counts[g], w[1]), g
    assert counts[3].tolist() == [0, 0, 0, 0] and bool(out[3, [2, 4, 6, 8, 11, 12]].isnan().all())
    again = ops.quality_pool(table, group, 4, P, L, flags)
    assert torch.equal(_bits(out), _bits(again[0])) and torch.equal(counts, again[1])
    alone = ops.quality_pool(table, None, 0, P, L, flags)
    assert _same_bits(alone[0][0], want_all[0]) and torch.equal(alone[1][0], want_all[1])


class _Lookup(torch.nn.Module):
    """a 'model' whose prediction for the feature value i is row i of a table of predictions: the evaluator's own code runs, and
    what it was given is known"""

    def __init__(self, loss, preds):
        super().__init__()
        self.loss, self.preds = loss, preds
        self.anchor = torch.nn.Parameter(torch.zeros(1, device='cuda'))

    def predict(self, x, route='auto'):
        idx = x[:, 0, 0].long()
        return {k: v[idx].contiguous() for k, v in self.preds.items()}


@pytest.mark.parametrize('capture', [False, True], ids=['eager', 'captured'])
def test_pooled_breakdown_of_the_evaluator(gpe, capture):
    """Evaluator.pooled against ops.quality_metrics on every group's garments as one batch, None by the gate table: group 0 'ok'
    garments, group 1 garments with an extra panel (no corr_ value at all), group 2 garments without a stitched-looking edge (the
    panel count is right, no stitches are detected: only the corr_stitch_ keys are None), group 3 empty, two ids out of range"""
    from gpe_amd import evaluation
    ops = gpe.ops
    fx = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    dc, lc = copy.deepcopy(fx['data_config']), fx['loss_config']
    P, L, S = dc['max_pattern_len'], dc['max_panel_len'], dc['max_num_stitches']
    sizes = (17, 17, 5)
    G = sum(sizes)
    preds, gt = quality_restate.make_batch(np.random.default_rng(77), G, P, L, S, dc, ['ok', 'extra', 'free0'])
    preds, gt = _cuda(preds), _cuda(gt)
    loss = gpe.metrics.ComposedPatternLoss(dc, copy.deepcopy(lc))
    model = _Lookup(loss, preds).eval()
    group = torch.arange(G) % 3
    group[6], group[G - 4] = 9, -1                       # (garments of groups 0 and 2: they count in 'all' only)
    batches, g0 = [], 0
    for B in sizes:
        idx = torch.arange(g0, g0 + B, device='cuda')
        batches.append((idx.float().view(B, 1, 1), _take(gt, idx)))
        g0 += B
    ev = evaluation.Evaluator(model, epoch=40, capture=capture, warmup=1)
    got = ev.run(iter(batches), groups=group, n_groups=4)            # an iterator: consumed as it comes, the table sized by `groups`
    assert set(ev.pooled) == {0, 1, 2, 3, 'all'} and ev.pooled_counts.shape == (5, 4) and ev.table.shape == (G, 16)
    names = [k for k in ops.QUALITY_KEYS if k in got]
    assert len(names) == 14
    subsets = {g: (group == g).nonzero().view(-1).cuda() for g in range(3)}
    subsets['all'] = torch.arange(G, device='cuda')
    for g, idx in subsets.items():
        out, counts = _quality(loss, _take(preds, idx), _take(gt, idx))
        out, counts = out.cpu().numpy(), counts.cpu().numpy()
        row = 4 if g == 'all' else g
        assert ev.pooled_counts[row].tolist() == counts.tolist(), g
        assert list(ev.pooled[g]) == names
        for k in names:
            j = R.GATES.get(k)
            want = None if j is not None and counts[j] <= 0 else out[ops.QUALITY_KEYS.index(k)]
            assert R.same(ev.pooled[g][k], want), (g, k, ev.pooled[g][k], want)
    corr = [k for k in names if k in R.GATES]
    assert len(corr) == 5
    assert all(ev.pooled[0][k] is not None for k in corr) and all(ev.pooled['all'][k] is not None for k in corr)
    assert all(ev.pooled[1][k] is None for k in corr) and ev.pooled[1]['rotation_l2'] is not None
    assert ev.pooled[2]['corr_rotation_l2'] is not None and ev.pooled[2]['corr_panel_shape_l2'] is not None
    assert ev.pooled[2]['corr_stitch_precision'] is None and ev.pooled[2]['corr_stitch_recall'] is None
    # the empty group: zero counts, None for the gated keys, the finalise kernel's 0 / 0 elsewhere
    assert ev.pooled_counts[3].tolist() == [0, 0, 0, 0] and all(ev.pooled[3][k] is None for k in corr)
    assert all(np.isnan(ev.pooled[3][k]) for k in names if k not in corr)
    # the reference-rule result of the same run, against loss.__call__ on the same batches
    per_batch = []
    with torch.no_grad():
        for x, g in batches:
            full, d, _ = loss(model.predict(x), dict(g), epoch=40)
            per_batch.append((full, d))
    R.assert_same(got, R.aggregate(per_batch), 'the run itself')
    for bad in (dict(total=G + 1), dict(groups=group[:-1])):
        with pytest.raises(ValueError, match='announced'):
            evaluation.Evaluator(model, epoch=40).run(iter(batches), **bad)
    with pytest.raises(ValueError, match='total = '):
        evaluation.Evaluator(model, epoch=40).run(iter(batches), groups=group, total=G - 1)


# ---- 4. the whole path ----------------------------------------------------------------------------------------------------------------
def _small_model(gpe):
    fx = torch.load(os.path.join(GOLDEN, 'full3d_small.pt'), weights_only=False)
    q = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    torch.manual_seed(0)
    model = gpe.nets.GarmentFullPattern3D(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(q['loss_config'])).cuda().eval()
    return model, fx, q


def _feature_batches(fx, q, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    out, at = [], 0
    for B in sizes:
        idx = [(at + i) % 10 for i in range(B)]
        out.append((torch.randn(B, fx['N'], 3, generator=g).cuda(), {k: v[idx].cuda() for k, v in q['gt'].items()}))
        at += B
    return out


def _host_rule(model, batches, epoch=40):
    per_batch = []
    with torch.no_grad():
        for x, gt in batches:
            full, d, _ = model.loss(model.predict(x), dict(gt), epoch=epoch)
            per_batch.append((full, d))
    return R.aggregate(per_batch)


def test_whole_path(gpe, math_mode):
    from gpe_amd import evaluation
    model, fx, q = _small_model(gpe)
    batches = _feature_batches(fx, q, (4, 4, 4, 2), 3)
    torch.manual_seed(7)
    want = _host_rule(model, batches)
    torch.manual_seed(7)
    ev = evaluation.Evaluator(model, epoch=40, capture=False)
    got = ev.run(batches)
    assert list(got)[0] == 'full_loss'
    R.assert_same(got, want, 'eager evaluator vs predict + loss.__call__')
    assert set(ev.pooled) == {'all'} and ev.pooled_counts.shape == (1, 4) and ev.table.shape == (14, 16)
    torch.manual_seed(7)
    cap = evaluation.Evaluator(model, epoch=40, capture=True)
    got_c = cap.run(batches)
    assert cap.captures == 1 and cap.replays == 1                       # two eager batches of 4, one replayed; the batch of 2 eager
    R.assert_same(got_c, got, 'captured vs eager')
    # one warm-up batch: the graph of size 4 is replayed twice (the start states are drawn afresh in front of every replay) and the
    # batch of 2 runs eagerly
    torch.manual_seed(7)
    cap1 = evaluation.Evaluator(model, epoch=40, capture=True, warmup=1)
    R.assert_same(cap1.run(batches), got, 'captured after one warm-up batch vs eager')
    assert cap1.captures == 1 and cap1.replays == 2 and torch.equal(cap1.table, ev.table)
    assert torch.equal(cap.table, ev.table)
    for k, v in ev.pooled['all'].items():
        assert R.same(cap.pooled['all'][k], v), k
    # the body of the capture must not have loosened the loss's own refusal
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    x, gt = batches[0]
    with torch.cuda.stream(side), torch.no_grad():
        preds = model.predict(x)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match='stream capture'):
            with torch.cuda.graph(g, stream=side):
                model.loss(preds, dict(gt), epoch=40)
    torch.cuda.synchronize()


def test_dict_of_folders(gpe):
    from gpe_amd import evaluation
    model, fx, q = _small_model(gpe)
    a, b = _feature_batches(fx, q, (4, 2), 11), _feature_batches(fx, q, (3, 3, 1), 12)
    torch.manual_seed(9)
    one = evaluation.Evaluator(model, epoch=40).run(a)
    two = evaluation.Evaluator(model, epoch=40).run(b)
    torch.manual_seed(9)
    ev = evaluation.Evaluator(model, epoch=40)
    both = ev.run({'skirt': a, 'tee': iter(b)}, groups=[0] * 6 + [1] * 7)
    assert list(both) == ['skirt', 'tee']
    R.assert_same(both['skirt'], one, 'skirt')
    R.assert_same(both['tee'], two, 'tee')
    assert set(ev.pooled) == {0, 1, 'all'} and ev.accumulator.last_batches.tolist() == [2, 3]
    assert ev.pooled_counts[:2].sum(0).tolist() == ev.pooled_counts[2].tolist()
    torch.manual_seed(9)
    short = evaluation.eval_metrics(model, {'skirt': a, 'tee': b})
    R.assert_same(short['tee'], two, 'eval_metrics')


# ---- 5. with the sampler ----------------------------------------------------------------------------------------------------------------
def _grid(nx, ny, bend):
    """nx x ny vertices on a bent sheet inside [-1, 1]^3, two triangles per cell (as tests/test_gpu_mesh_sample.py builds them)"""
    u, v = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), indexing='ij')
    verts = np.stack([0.9 * np.cos(bend * u) * (0.4 + 0.6 * u), 0.9 * np.sin(bend * u) * (0.4 + 0.6 * u), 1.6 * v - 0.8 + 0.1 * u], axis=-1)
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    return verts.reshape(-1, 3).astype(np.float32), faces.astype(np.int64)


def test_with_the_sampler(gpe, math_mode):
    from gpe_amd import evaluation
    model, fx, q = _small_model(gpe)
    meshes = []
    for m in range(6):
        v, f = _grid(5 + m, 4, 1.0 + 0.5 * m)
        meshes.append((v, f, np.arange(len(v)) % 3))
    sampler = gpe.staging.MeshPointSampler(meshes, None, mesh_samples=fx['N'], seed=1)
    index = [[0, 1, 2, 3], [4, 5, 0, 2], [3, 1, 5, 4], [2, 0]]
    batches = [(torch.tensor(i, device='cuda'), {k: v[i].cuda() for k, v in q['gt'].items()}) for i in index]
    runs = []
    for capture in (False, False, True):
        torch.manual_seed(13)
        ev = evaluation.Evaluator(model, sampler, epoch=40, capture=capture)
        runs.append((ev.run(batches, seed=3), ev.table.clone()))
    R.assert_same(runs[1][0], runs[0][0], 'two runs with one seed')
    assert torch.equal(runs[1][1], runs[0][1])
    R.assert_same(runs[2][0], runs[0][0], 'captured')
    torch.manual_seed(13)
    cap1 = evaluation.Evaluator(model, sampler, epoch=40, capture=True, warmup=1)          # two replays: the draw counter advances on the device
    R.assert_same(cap1.run(batches, seed=3), runs[0][0], 'captured, replayed twice')
    assert cap1.replays == 2 and torch.equal(cap1.table, runs[0][1])
    torch.manual_seed(13)
    other = evaluation.Evaluator(model, sampler, epoch=40).run(batches, seed=4)
    assert not R.same(other['pattern_loss'], runs[0][0]['pattern_loss'])              # another seed: other clouds
    # the sampler's status is looked at once, at the end: an index outside the set is reported by run(), after all batches ran
    bad = batches[:1] + [(torch.tensor([1, 77], device='cuda'), batches[3][1])]
    ev = evaluation.Evaluator(model, sampler, epoch=40)
    with pytest.raises(ValueError, match='status -2'):
        ev.run(bad, seed=3)
    assert ev.accumulator.last_batches.tolist() == [2]
    with pytest.raises(ValueError, match='sampler'):
        evaluation.Evaluator(model, None, epoch=40).run(batches)


# ---- 6. the pair classifier -------------------------------------------------------------------------------------------------------------
def test_pair_classifier(gpe):
    from gpe_amd import evaluation
    fx = torch.load(os.path.join(GOLDEN, 'stitch_train_small.pt'), weights_only=False)
    torch.manual_seed(11)
    model = gpe.nets.StitchOnEdge3DPairs(fx['data_config'], dict(fx['nn_config']), {}).cuda().eval()
    pairs, labels = fx['pairs'].cuda(), fx['labels'].cuda()
    batches = [(pairs[i:i + 1], labels[i:i + 1]) for i in range(3)]
    per_batch = []
    with torch.no_grad():
        for x, y in batches:
            full, d, _ = model.loss(model.predict(x), y)
            per_batch.append((full, d))
    want = R.aggregate(per_batch)
    assert list(want) == ['full_loss', 'edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall']
    ev = evaluation.Evaluator(model)
    R.assert_same(ev.run(batches), want, 'pair classifier')
    assert ev.pooled is None and ev.table is None
    R.assert_same(evaluation.Evaluator(model, capture=True, warmup=1).run(batches), want, 'pair classifier, captured')
