"""-m gpu: the edge-pair classifier scored on predicted patterns over a whole set on the device (csrc/gpe_framework_eval.hip through
ops.FrameworkAccumulator and evaluation.FrameworkEvaluator) against the numpy restatement (tests/framework_eval_restate.py), which
tests/test_framework_eval_host.py pins to the reference's own numbers.

Bars.  The kernel alone and the pooling are BIT-equal to the restatement: a garment's ratios are one correctly rounded fp32 division
of exact integers on both sides, its loss one fp64 division rounded once, the folds sequential adds in the same order.  The chain
(decode -> place -> classifier) is exact in every counter where every fp64 logit of the restatement keeps the margin of
tests/test_gpu_stitch_eval.py from 0 (4 tol, tol = 1e-4 max(1, max |logit|)) and the two best positives of an edge keep it from each
other; the loss is then within that test's bar, tol + 2^-20 max(1, loss), per garment and so for their mean."""
import os

import numpy as np
import pytest
import torch

import eval_restate as ER
import framework_eval_restate as FW
import stitch_pairs_restate as R
import test_framework_eval_host as H          # the chain case (8 garments) and its restatement: computed once, shared
import test_gpu_eval as GE                    # feature batches with ground truth, the sampler's meshes (helpers only)
import test_gpu_pattern_place as PP           # the predict_garment models: the small pattern model and the shipped classifier

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
REL = 2.0 ** -20


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


# ---- hand-built garments: every state, the precedence, every zero denominator -----------------------------------------------------------
CASES = [dict(), dict(gt_panels=4), dict(flags=(1, 0, 0)), dict(flags=(0, 2, 0)), dict(ns=0), dict(first=0), dict(first=2),
         dict(counts=(0,) * 6, loss_sum=0.0), dict(counts=(10, 10, 0, 0, 3, 0)), dict(counts=(10, 7, 0, 3, 0, 0)), dict(sel=0),
         dict(flags=(0, 0, 4), ns=0, counts=(0,) * 6), dict(ns=0, counts=(0,) * 6), dict(first=0, gt_panels=1),
         dict(counts=(3, 1, 0, 0, 1, 0), loss_sum=1.0)]


def _hand(B, seed, slot):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(B):
        k = dict(CASES[(i + seed) % len(CASES)]) if i % 2 == 0 else {}
        if 'counts' not in k:
            pairs = int(rng.integers(1, 50000))
            pred, gtp = int(rng.integers(0, min(pairs, 300) + 1)), int(rng.integers(0, min(pairs, 40) + 1))
            tp = int(rng.integers(0, min(pred, gtp) + 1))
            sel = int(rng.integers(0, 30))
            k['counts'] = (pairs, int(rng.integers(0, pairs + 1)), tp, pred, gtp, int(rng.integers(0, min(sel, gtp) + 1)))
            k.setdefault('sel', sel)
            k['loss_sum'] = float(rng.uniform(0, 2.0 * pairs))
        k.setdefault('panels', int(rng.integers(1, 4)))
        k.setdefault('gt_panels', k['panels'] if rng.random() < 0.6 else k['panels'] + 1)
        out.append(H._g(slot=slot, **k))
    return out


def _tensors(garments):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()      # noqa: E731
    ev = {'counts': i32([g['counts'] for g in garments]), 'loss_sum': torch.tensor([g['loss_sum'] for g in garments], dtype=torch.float64).cuda(),
          'num_stitches': i32([g['num_selected'] for g in garments])}
    dec = {'num_stitches': i32([g['num_stitches'] for g in garments]), 'first_invalid': i32([g['first_invalid'] for g in garments]),
           'num_panels': i32([g['num_panels'] for g in garments]), 'num_edges': i32([g['num_edges'] for g in garments]),
           'place_flags': i32([g['place_flags'] for g in garments])}
    return ev, dec, torch.tensor([g['gt_num_panels'] for g in garments]).cuda()


def _run_batches(gpe, batches, slots):
    """batches: [(slot, garments)] in visiting order -> the accumulator after all of them"""
    acc = gpe.ops.FrameworkAccumulator(slots=slots, total=sum(len(g) for _, g in batches), device='cuda')
    for slot, garments in batches:
        acc.set_slot(slot)
        acc.add(*_tensors(garments))
    return acc


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind == 'f':
        ok = (FW.bits(got) == FW.bits(want)) | (np.isnan(got) & np.isnan(want))        # as eval_restate.same compares
    else:
        ok = got == want
    assert ok.all(), (what, np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])


@pytest.mark.parametrize('B', [1, 2, 63, 64, 65, 200])
def test_kernel_alone_is_bit_equal_to_the_restatement(gpe, B):
    batches = [(slot, _hand(B, 10 * B + n, slot)) for n, slot in enumerate((2, 0, 2, 1))]          # three rows in mixed order
    acc = _run_batches(gpe, batches, 3)
    rows = acc.read()
    sums, cnt, skipped, records = FW.fold([g for _, gs in batches for g in gs], slots=3)
    _same_bits(acc.last_sums, sums, 'sums')
    _same_bits(acc.last_counts, cnt, 'cnt')
    _same_bits(acc.last_skipped, skipped, 'skipped')
    _same_bits(acc.table.cpu().numpy(), records, 'records')
    want = FW.result(sums, cnt, skipped)
    for s in range(3):
        for name in FW.SETS:
            ER.assert_same(rows[s][name], want[s][name], (s, name))
        assert rows[s]['skipped'] == want[s]['skipped']
    assert acc.rows == 4 * B and int(acc.status.cpu()) == 0
    if B >= 63:
        states = records[:, 0].astype(int).tolist()
        assert set(states) == {0, 1, 2, 3} and skipped[:, 3].sum() > 0 and cnt[1].sum() > 0


def test_slot_word_out_of_range_sets_the_status_and_changes_nothing(gpe):
    garments = _hand(65, 5, 0)
    acc = _run_batches(gpe, [(1, garments)], 2)
    before, table = acc.state.clone(), acc.table.clone()
    for bad in (2, -1, 1 << 20):
        acc.slot.fill_(bad)
        acc.add(*_tensors(_hand(65, 6, 0)), records=torch.zeros(65, 10, dtype=torch.float64, device='cuda'))
        torch.cuda.synchronize()
        assert torch.equal(acc.state[:-1], before[:-1]) and int(acc.status.cpu()) == 1 and torch.equal(acc.table, table)
        with pytest.raises(RuntimeError, match='slot word outside'):
            acc.read()
        acc.status.zero_()
    acc.set_slot(1)
    assert acc.read()[1]['stitch'] == FW.result(*FW.fold(_hand(65, 5, 1), slots=2)[:3])[1]['stitch']
    with pytest.raises(ValueError, match='more garments'):
        acc.add(*_tensors(_hand(1, 1, 0)))
    with pytest.raises(ValueError, match='set_slot'):
        acc.set_slot(2)


def test_two_runs_and_a_cu_reservation_give_the_same_bits(gpe):
    batches = [(slot, _hand(B, 77 + n, slot)) for n, (slot, B) in enumerate(((1, 200), (0, 65), (1, 3)))]
    groups = torch.arange(268, dtype=torch.int32).cuda() % 5

    def once():
        acc = _run_batches(gpe, batches, 2)
        return [acc.state, acc.table] + list(acc.pool(groups, 3))
    a, b = once(), once()
    prev = gpe._lib.set_reserved_cus(16)
    try:
        c = once()
    finally:
        gpe._lib.set_reserved_cus(prev)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and torch.equal(x.view(torch.uint8), z.view(torch.uint8))


# ---- pooling ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_groups', [0, 3])
@pytest.mark.parametrize('G', [1, 64, 65, 130])
def test_pool_is_bit_equal_to_the_restatement(gpe, G, n_groups):
    garments = _hand(G, 1000 + G, 0)
    records = FW.fold(garments)[3]
    rng = np.random.default_rng(G)
    groups = rng.choice([-1, 0, 2, 3, 7], size=G).astype(np.int32) if n_groups else None          # group 1 stays empty; ids out of range
    acc = gpe.ops.FrameworkAccumulator(slots=1, total=1, device='cuda')
    table = torch.from_numpy(records).cuda()
    got = acc.pool(torch.from_numpy(groups).cuda() if n_groups else None, n_groups, table=table)
    totals, loss, ratios = FW.pool(records, groups, n_groups)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float64 and got[2].dtype == torch.float32
    _same_bits(got[0].cpu().numpy(), totals, 'totals')
    _same_bits(got[1].cpu().numpy(), loss, 'loss')
    _same_bits(got[2].cpu().numpy(), ratios, 'ratios')
    if n_groups:
        assert not totals[1].any() and not got[0][1].any() and not got[1][1].any() and not got[2][1].any()       # an empty group: zeros
        assert totals[:3, :, 7].sum() <= totals[3, 0, 7] * 2
    with pytest.raises(ValueError, match='groups'):
        acc.pool(None, 2, table=table)
    with pytest.raises(ValueError, match='table must be'):
        acc.pool(None, 0, table=table[:, :9].contiguous())


# ---- the chain: decode -> place -> classifier -> accumulate ------------------------------------------------------------------------------
def _evaluator(gpe, dc, stats, known, **kw):
    model, _, _ = GE._small_model(gpe)
    stitch = gpe.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    stitch.load_state_dict(known['state_dict'])                                            # the shipped classifier weights
    return gpe.evaluation.FrameworkEvaluator(model, stitch.cuda().eval(), dc, stats, **kw)


def _slice(d, idx):
    return {k: v[idx].cuda() for k, v in d.items()}


def _pass(ev, preds, gt, sizes, groups=None, n_groups=None):
    """the 8 garments cut into batches of `sizes` -> (result, pooled, records on the host)"""
    ev.begin(total=sum(sizes))
    at = 0
    for B in sizes:
        idx = slice(at, at + B)
        ev.add_predictions(_slice(preds, idx), _slice(gt, idx))
        at += B
    rows = ev.finish(groups, n_groups)
    return rows[0], ev.pooled, ev.records.cpu().numpy()


def _pooled_same(a, b):
    assert set(a) == set(b)
    for r in a:
        for name in FW.SETS:
            ER.assert_same(a[r][name], b[r][name], (r, name))
            assert a[r]['counts'][name].keys() == b[r]['counts'][name].keys()
            for k, v in a[r]['counts'][name].items():
                assert np.float64(v).view(np.int64) == np.float64(b[r]['counts'][name][k]).view(np.int64), (r, name, k)


def test_chain_against_the_restatement(gpe):
    preds, gt, dc, known, stats, garments, detail = H.chain_case()
    ev = _evaluator(gpe, dc, stats, known)
    res, pooled, records = _pass(ev, preds, gt, [8])
    # which garments compare exactly: the restatement alone decides
    exact = []
    for g, d in zip(garments, detail):
        tol = R.tol_of(d['logits'])
        m0, gap = R.margins(d['pairs'], d['logits'])
        exact.append(m0 >= 4 * tol and gap >= 4 * tol)
    assert sum(not e for e in exact) <= 1, exact
    want_records = FW.fold(garments)[3]
    assert records.shape == (8, 10)
    bars = [0.0] * 8
    for b, (g, d) in enumerate(zip(garments, detail)):
        print('garment %d: device record %s' % (b, records[b].tolist()))
        pairs = g['counts'][0]
        assert records[b, [0, 1, 3]].tolist() == want_records[b, [0, 1, 3]].tolist(), b       # state, corr, pairs: no logit decides them
        if pairs:
            loss, loss64 = records[b, 2] / pairs, g['loss_sum'] / pairs
            bars[b] = R.tol_of(d['logits']) + REL * max(1.0, loss64)
            print('garment %d: loss %.9g, restated %.9g, |difference| %.3g (bar %.3g)' % (b, loss, loss64, abs(loss - loss64), bars[b]))
            assert abs(loss - loss64) < bars[b], b
        if exact[b]:
            assert records[b, 3:].tolist() == want_records[b, 3:].tolist(), (b, records[b].tolist(), want_records[b].tolist())
    # the folded result: the fold of the device's OWN records, bit for bit ...
    own = [FW.garment(records[b, 3:9], records[b, 2], records[b, 9], g['num_stitches'], g['first_invalid'], g['num_panels'],
                      g['gt_num_panels'], g['num_edges'], g['place_flags']) for b, g in enumerate(garments)]
    assert [FW.state(g) for g in own] == records[:, 0].astype(int).tolist() and [float(FW.corr(g)) for g in own] == records[:, 1].tolist()
    sums, cnt, skipped, _ = FW.fold(own)
    want_own = FW.result(sums, cnt, skipped)[0]
    for name in FW.SETS:
        ER.assert_same(res[name], want_own[name], name)
    assert res['skipped'] == want_own['skipped'] == {'bad_rotation': 0, 'no_stitches': 1, 'no_pairs': 1, 'wrong_panel_count': 2}
    totals, loss, ratios = FW.pool(records)
    for i, name in enumerate(FW.SETS):
        ER.assert_same(pooled['all'][name], dict(zip(FW.METRICS, ratios[0, i])), name)
        assert [pooled['all']['counts'][name][k] for k in FW.TOTALS] == totals[0, i].tolist()
        assert pooled['all']['counts'][name]['loss_sum'] == loss[0, i]
    # ... and within the stitch-eval loss tolerance of the restatement: every member's value moves by less than its own bar, so
    # their mean by less than the mean of the bars; rounding a value to fp32 and the n adds and one division of the fold are one
    # fp32 rounding each of at most S = sum |v_i| on either side (tests/test_framework_eval_host.py): 3 * 2^-24 * S covers both.
    # The ratios are bit-equal where every garment's counters are.
    want = FW.result(*FW.fold(garments)[:3])[0]
    for name, members in (('stitch', [FW.state(g) == 0 for g in garments]),
                          ('stitch_corr', [FW.state(g) == 0 and FW.corr(g) for g in garments])):
        n = sum(members)
        S = sum(abs(float(FW.values(g)[0])) for g, m in zip(garments, members) if m)
        tol = sum(b for b, m in zip(bars, members) if m) / n + 3 * 2.0 ** -24 * S
        for k in FW.KEYS:
            got, w = float(res[name][k]), float(want[name][k])
            if k in ('full_loss', 'edge_pair_class_loss'):
                print('%s %s: %.9g, restated %.9g, |difference| %.3g (bar %.3g)' % (name, k, got, w, abs(got - w), tol))
                assert abs(got - w) < tol, (name, k)
            elif all(exact):
                assert ER.same(res[name][k], want[name][k]), (name, k)


def test_batching_does_not_change_the_result_and_folders_are_rows(gpe):
    preds, gt, dc, known, stats, garments, detail = H.chain_case()
    ev = _evaluator(gpe, dc, stats, known, shape_metrics=False)
    groups = [0, 1, 0, 5, 1, 1, 0, 1]
    res, pooled, records = _pass(ev, preds, gt, [8], groups, 2)
    assert set(pooled) == {0, 1, 'all'}
    for sizes in ([5, 3], [1] * 8):
        r2, p2, rec2 = _pass(ev, preds, gt, sizes, groups, 2)
        _same_bits(rec2, records, sizes)
        _pooled_same(p2, pooled)
        for name in FW.SETS:
            ER.assert_same(r2[name], res[name], (sizes, name))
        assert r2['skipped'] == res['skipped']
    # a dict of two folders: two rows, each equal to a run of its own
    ev.begin(total=8, slots=2)
    ev.accumulator.set_slot(0)
    ev.add_predictions(_slice(preds, slice(0, 5)), _slice(gt, slice(0, 5)))
    ev.accumulator.set_slot(1)
    ev.add_predictions(_slice(preds, slice(5, 8)), _slice(gt, slice(5, 8)))
    rows = ev.finish()
    for row, idx in zip(rows, (slice(0, 5), slice(5, 8))):
        ev.begin(total=idx.stop - idx.start)
        ev.add_predictions(_slice(preds, idx), _slice(gt, idx))
        alone = ev.finish()[0]
        for name in FW.SETS:
            ER.assert_same(row[name], alone[name], name)
        assert row['skipped'] == alone['skipped']


def test_run_end_to_end(gpe):
    from gpe_amd import evaluation
    fx, model, stitch, stats = PP._models(gpe)
    q = H._load('quality_lstm_e40.pt')                       # ground truth with stitches and panel counts
    dc = fx['data_config']
    batches = GE._feature_batches(fx, q, (4, 3), 21)
    torch.manual_seed(13)
    shape = evaluation.Evaluator(model, epoch=40)
    want_shape = shape.run(batches)
    torch.manual_seed(13)
    ev = evaluation.FrameworkEvaluator(model, stitch, dc, stats, epoch=40)
    got = ev.run(batches)
    assert list(got) == ['shape', 'stitch', 'stitch_corr', 'skipped']
    print('run: counted %s, skipped %s' % (ev.accumulator.last_counts.tolist(), got['skipped']))
    assert ev.accumulator.last_counts[0, 0] > 0              # some garment is counted: the comparisons below are about numbers
    ER.assert_same(got['shape'], want_shape, 'shape')
    assert torch.equal(ev.shape.table, shape.table)
    for k, v in shape.pooled['all'].items():
        assert ER.same(ev.shape.pooled['all'][k], v), k
    run_pooled, run_records = ev.pooled, ev.records.cpu().numpy()
    # the stitch entries: add_predictions on the predictions model.predict returns
    torch.manual_seed(13)
    ev2 = evaluation.FrameworkEvaluator(model, stitch, dc, stats, shape_metrics=False, epoch=40)
    ev2.begin(total=7)
    for x, gt in batches:
        ev2.add_predictions(model.predict(x), gt)
    alone = ev2.finish()[0]
    for name in FW.SETS:
        ER.assert_same(got[name], alone[name], name)
    assert got['skipped'] == alone['skipped'] and sum(got['skipped'].values()) + ev.accumulator.last_counts[1, 0] == 7
    _same_bits(ev2.records.cpu().numpy(), run_records, 'records')
    _pooled_same(ev2.pooled, run_pooled)
    # a dict of folders gives a dict of results; eval_framework is the shortcut
    torch.manual_seed(13)
    both = evaluation.eval_framework(model, stitch, dc, stats, {'a': batches[:1], 'b': iter(batches[1:])}, epoch=40, total=7)
    assert list(both) == ['a', 'b'] and list(both['a']) == ['shape', 'stitch', 'stitch_corr', 'skipped']
    torch.manual_seed(13)
    first = evaluation.FrameworkEvaluator(model, stitch, dc, stats, epoch=40).run(batches[:1])
    ER.assert_same(both['a']['shape'], first['shape'], 'folder a, shape')
    for name in FW.SETS:
        ER.assert_same(both['a'][name], first[name], name)


def test_run_with_the_sampler(gpe):
    """batches of garment indices: the clouds are drawn on the device, and with one seed the first stage's result is Evaluator's"""
    from gpe_amd import evaluation
    fx, model, stitch, stats = PP._models(gpe)
    q = H._load('quality_lstm_e40.pt')                       # ground truth with stitches and panel counts
    meshes = []
    for m in range(6):
        v, f = GE._grid(5 + m, 4, 1.0 + 0.5 * m)
        meshes.append((v, f, np.arange(len(v)) % 3))
    sampler = gpe.staging.MeshPointSampler(meshes, None, mesh_samples=fx['N'], seed=1)
    index = [[0, 1, 2, 3], [4, 5, 0]]
    batches = [(torch.tensor(i, device='cuda'), {k: v[i].cuda() for k, v in q['gt'].items()}) for i in index]
    torch.manual_seed(13)
    want = evaluation.Evaluator(model, sampler, epoch=40).run(batches, seed=3)
    torch.manual_seed(13)
    ev = evaluation.FrameworkEvaluator(model, stitch, fx['data_config'], stats, sampler, epoch=40)
    got = ev.run(batches, groups=[0, 1, 0, 1, 0, 1, 5], n_groups=2, seed=3)
    ER.assert_same(got['shape'], want, 'shape, sampled clouds')
    print('run with the sampler: counted %s, skipped %s' % (ev.accumulator.last_counts.tolist(), got['skipped']))
    assert ev.accumulator.last_counts[0, 0] > 0
    assert set(ev.pooled) == {0, 1, 'all'} and ev.records.shape == (7, 10)
    torch.manual_seed(13)
    again = ev.run(batches, groups=[0, 1, 0, 1, 0, 1, 5], n_groups=2, seed=3)
    for name in FW.SETS:
        ER.assert_same(again[name], got[name], name)
    with pytest.raises(ValueError, match='sampler'):
        evaluation.FrameworkEvaluator(model, stitch, fx['data_config'], stats, epoch=40).run(batches)


def test_one_add_inside_a_graph_on_a_single_stream(gpe):
    """no hidden host read: one add() captured alone, replayed twice = two eager calls"""
    garments = _hand(65, 31, 0)
    ev_out, dec, gtp = _tensors(garments)
    eager = gpe.ops.FrameworkAccumulator(slots=2, total=65, device='cuda')
    captured = gpe.ops.FrameworkAccumulator(slots=2, total=65, device='cuda')
    rows_e = torch.zeros(65, 10, dtype=torch.float64, device='cuda')
    rows_c = torch.zeros(65, 10, dtype=torch.float64, device='cuda')
    eager.set_slot(1)
    captured.set_slot(1)
    eager.add(ev_out, dec, gtp, records=rows_e)
    eager.add(ev_out, dec, gtp, records=rows_e)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        side.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            captured.add(ev_out, dec, gtp, records=rows_c)
        cg.replay()
        cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.state, eager.state) and torch.equal(rows_c, rows_e)
    assert int(captured.cnt[0, 1].cpu()) == 2 * sum(FW.state(g) == 0 for g in garments) > 0


# ---- gates --------------------------------------------------------------------------------------------------------------------------------
def test_gates(gpe):
    preds, gt, dc, known, stats, garments, detail = H.chain_case()
    tags = _evaluator(gpe, dc, stats, known, labels='tags', shape_metrics=False)
    tags.begin(total=8)
    d = tags.add_predictions(_slice(preds, slice(0, 8)), {'num_panels': gt['num_panels'].cuda()})      # no 'stitches' needed
    res = tags.finish()[0]
    assert d.placed is not None and set(res) == {'stitch', 'stitch_corr', 'skipped'}
    assert sum(res['skipped'].values()) + tags.accumulator.last_counts[1, 0] == 8
    ev = _evaluator(gpe, dc, stats, known)
    ev.begin(total=8)
    with pytest.raises(ValueError, match="no 'stitches'"):
        ev.add_predictions(_slice(preds, slice(0, 8)), {'num_panels': gt['num_panels'].cuda()})
    with pytest.raises(ValueError, match="no 'num_panels'"):
        ev.add_predictions(_slice(preds, slice(0, 8)), {'stitches': gt['stitches'].cuda()})
    with pytest.raises(ValueError, match='no batch to evaluate'):
        ev.finish()
    for m in (ev.model, ev.stitch_model):
        m.train()
        with pytest.raises(RuntimeError, match=r'call \.eval\(\) first'):
            ev.begin(total=8)
        with pytest.raises(RuntimeError, match=r'call \.eval\(\) first'):
            ev.run([(preds['outlines'], gt)], total=8)
        m.eval()
    # argument errors of the accumulator come before any launch
    acc = gpe.ops.FrameworkAccumulator(slots=1, total=4, device='cuda')
    ev_out, dec, gtp = _tensors(_hand(4, 1, 0))
    with pytest.raises(ValueError, match='counts must be int32'):
        acc.add(dict(ev_out, counts=ev_out['counts'].long()), dec, gtp)
    with pytest.raises(ValueError, match='is missing'):
        acc.add(ev_out, {k: v for k, v in dec.items() if k != 'place_flags'}, gtp)
    with pytest.raises(ValueError, match='gt_num_panels'):
        acc.add(ev_out, dec, gtp[:3])
    with pytest.raises(ValueError, match='num_edges'):
        acc.add(ev_out, dict(dec, num_edges=torch.zeros(4, 65, dtype=torch.int32, device='cuda')), gtp)
    with pytest.raises(RuntimeError, match='no CPU path'):
        acc.add({k: v.cpu() for k, v in ev_out.items()}, {k: v.cpu() for k, v in dec.items()}, gtp.cpu())
    with pytest.raises(ValueError, match='no garment has been added'):
        acc.pool()
    assert acc.rows == 0 and not acc.state.any()
