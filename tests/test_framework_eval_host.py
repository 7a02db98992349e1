"""not-gpu: the two-stage evaluation pass (include/gpe_hip_framework.h, ops.FrameworkAccumulator, DecodedPatterns.label_stitches,
evaluation.FrameworkEvaluator) as far as it goes without a device:
  (1) the restatement (tests/framework_eval_restate.py) against the reference's own `_eval_metrics_per_loader` on one-garment batches
      (tests/golden/framework_eval_small.pt, scripts/make_framework_eval_golden.py), within a tolerance derived below;
  (2) the rules on hand-built garments: every state, their precedence, zero denominators, first_invalid = 0, the corr set, per-slot
      separation, the pooled rows;
  (3) the whole per-garment chain restated on tests/golden/pattern_decode_given.pt and two hand-made garments (states 2 and 3);
  (4) the C ABI: gpe_hip_framework.h parses and binds through _lib.FRAMEWORK_HEADERS, both symbols are exported, -22 on bad arguments
      before any pointer is touched;
  (5) the Python refusals that need no device."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gpe_amd
from gpe_amd import _lib, evaluation, ops, patterns
import eval_restate as ER
import framework_eval_restate as FW
import stitch_eval_restate as EV

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
SYMBOLS = ('gpe_framework_eval_add', 'gpe_framework_eval_pool')
U = 2.0 ** -24            # one float32 rounding, relative


def _load(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


# ---- (1) the reference's own numbers ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_garments():
    """the garments of stitch_eval_*.pt as the kernel would see them, from the reference's stored logits: -> (tags, garments,
    per-garment {'bound', 'ref_loss'})"""
    fw = _load('framework_eval_small.pt')
    tags, garments, info = [], [], []
    for tag in fw['tags'] + fw['left_out']:
        ev, fx = _load('stitch_eval_%s.pt' % tag), _load('stitch_pairs_%s.pt' % tag)
        pairs = [tuple(int(v) for v in row) for row in fx['ref_order'].tolist()]
        plants = [(tuple(a), tuple(b)) for a, b in ev['plants']]
        logits = fx['ref_logits'].numpy()
        got = EV.evaluate(pairs, logits, plants)
        c = got['counts']
        n_panels = int((fx['num_edges'] > 0).sum())
        correct = tag in fw['tags'] and fw['correct'][fw['tags'].index(tag)]
        garments.append(FW.garment([c[k] for k in FW.COUNTS], got['loss_sum'], c['selected'], len(plants), -1, n_panels,
                                   n_panels if correct else n_panels + 1, fx['num_edges'].tolist(), [0] * len(fx['num_edges'])))
        tags.append(tag)
        info.append({'bound': EV.reference_arithmetic_bound(logits), 'ref_loss': ev['ref_loss_dict']['edge_pair_class_loss']})
    return fw, tags, garments, info


def test_restatement_against_the_references_own_fold():
    """The reference's dict is sum(list) / len(list) over the per-garment float32 values of its ComposedLoss, one garment per batch.

    Accuracy, precision, recall: a garment's value is ONE float32 division of two small integers on both sides (torch's float32
    division and numpy's are correctly rounded; the reference's Python 0 on an empty denominator is the same number), so the lists
    are bit-equal and only the fold can differ: n - 1 adds and one division.  The fixture records the type of every returned value:
    float32, so the reference's sum() ran in float32 like ours and these three keys are asserted BIT-EQUAL.  The tolerance below is
    kept as the statement of what could differ otherwise.  The restatement rounds each to float32; had the
    reference's sum() run in float64 (it depends on what `0 + array` promotes to), every add and the division would differ from
    ours by at most one float32 rounding of a partial sum <= S = sum |v_i|: at most U S for each of the n - 1 adds, then divided by
    n, plus U S / n for the division — together <= U S, with U = 2^-24.  That is the tolerance of these keys.

    The loss: the restatement's per-garment value is the exact fp64 mean of the BCE terms rounded once to float32 (U |v_i|); the
    reference's is torch's float32 BCEWithLogitsLoss, which lies within EV.reference_arithmetic_bound(logits) of the exact mean for
    its float32 TERMS, and whose float32 mean over the terms tests/test_stitch_eval_host.py pins within 1e-6 relative of the
    restated float32 arithmetic (the bar that test asserts per garment).  So |v_i - ref_i| <= bound_i + 1e-6 ref_i + U |v_i|, the
    mean of n such garments moves by their mean, and the fold adds U S as above."""
    fw, tags, garments, info = _reference_garments()
    assert fw['left_out'] == ['none'] and tags[-1] == 'none' and FW.state(garments[-1]) == FW.NO_STITCHES      # datasets.py:1149
    assert [FW.state(g) for g in garments[:-1]] == [FW.COUNTED] * 5 and [FW.corr(g) for g in garments[:-1]] == fw['correct']
    sums, cnt, skipped, _ = FW.fold(garments)
    res = FW.result(sums, cnt, skipped)[0]
    assert cnt.tolist() == [[5], [3]] and res['skipped'] == {'bad_rotation': 0, 'no_stitches': 1, 'no_pairs': 0, 'wrong_panel_count': 2}
    for name, ref, members in (('stitch', fw['ref_all'], [True] * 5), ('stitch_corr', fw['ref_corr'], fw['correct'])):
        assert set(ref) == set(FW.KEYS[:5])
        vals = [FW.values(g) for g, m in zip(garments, members) if m]
        n = len(vals)
        for j, k in enumerate(FW.KEYS[:5]):
            S = float(sum(abs(float(v[j])) for v in vals))
            tol = U * S
            if j < 2:
                tol += sum(i['bound'] + 1e-6 * i['ref_loss'] + U * abs(float(v[j])) for i, v, m in zip(info, vals, members) if m) / n
            got = float(res[name][k])
            print('%-11s %-22s restated %.9g  reference %.9g  |difference| %.3g  (tolerance %.3g)'
                  % (name, k, got, ref[k], abs(got - ref[k]), tol))
            assert abs(got - ref[k]) <= tol, (name, k)
            if j >= 2:
                # the fixture records that the reference's sum() ran in float32: then the fold is ours step for step, bit for bit
                assert fw['ref_all_types'][k] == fw['ref_corr_types'][k] == 'float32:float32'
                assert ER.same(res[name][k], np.float32(ref[k])), (name, k)
    # the keys the reference does not have score the selected stitches: present, finite, in 0 .. 1
    for k in FW.KEYS[5:]:
        assert 0.0 <= float(res['stitch'][k]) <= 1.0


# ---- (2) the rules by hand --------------------------------------------------------------------------------------------------------------
def _g(counts=(10, 8, 2, 4, 3, 1), loss_sum=5.0, sel=2, ns=3, first=-1, panels=3, gt_panels=3, ne=(4, 0, 5), flags=(0, 0, 0), slot=0):
    return FW.garment(counts, loss_sum, sel, ns, first, panels, gt_panels, ne, flags, slot)


def test_states_and_their_precedence():
    assert FW.state(_g()) == FW.COUNTED and FW.corr(_g())
    assert FW.state(_g(flags=(1, 0, 0))) == FW.BAD_ROTATION
    assert FW.state(_g(flags=(0, 1, 0))) == FW.COUNTED                   # a flag on an empty panel: nobody places it
    assert FW.state(_g(ns=0)) == FW.NO_STITCHES
    assert FW.state(_g(first=0)) == FW.NO_STITCHES                       # the first stitch is invalid: none is kept
    assert FW.state(_g(first=2)) == FW.COUNTED and FW.n_labels(_g(first=2)) == 2
    assert FW.state(_g(counts=(0, 0, 0, 0, 0, 0), loss_sum=0.0)) == FW.NO_PAIRS
    # precedence: rotation, then stitches, then pairs
    assert FW.state(_g(flags=(0, 0, 4), ns=0, counts=(0,) * 6)) == FW.BAD_ROTATION
    assert FW.state(_g(ns=0, counts=(0,) * 6)) == FW.NO_STITCHES
    assert not FW.corr(_g(gt_panels=4))


def test_values_and_zero_denominators():
    f = np.float32
    v = FW.values(_g())
    assert v == [f(0.5), f(0.5), f(8) / f(10), f(2) / f(4), f(2) / f(3), f(1) / f(2), f(1) / f(3)]
    assert all(x.dtype == np.float32 for x in v)
    v = FW.values(_g(counts=(10, 10, 0, 0, 0, 0), sel=0))               # nothing predicted, nothing labelled, nothing selected
    assert v[2:] == [f(1), f(0), f(0), f(0), f(0)]
    v = FW.values(_g(counts=(3, 1, 0, 0, 1, 0), loss_sum=1.0))
    assert v[0] == f(1.0 / 3.0) and v[3] == 0 and v[4] == 0


def test_fold_is_sequential_float32_per_slot_and_set():
    f = np.float32
    gs = [_g(slot=1), _g(counts=(7, 3, 1, 1, 2, 1), loss_sum=0.7, gt_panels=5, slot=1), _g(ns=0, slot=1), _g(flags=(2, 0, 0), slot=0),
          _g(counts=(3, 3, 0, 0, 0, 0), loss_sum=0.1, slot=0), _g(counts=(0,) * 6, slot=2), _g(counts=(9, 1, 1, 8, 1, 0), slot=1)]
    sums, cnt, skipped, records = FW.fold(gs, slots=3)
    assert cnt.tolist() == [[1, 3, 0], [1, 2, 0]]
    assert skipped.tolist() == [[1, 0, 0, 0], [0, 1, 0, 1], [0, 0, 1, 0]]
    a, b, c = FW.values(gs[0]), FW.values(gs[1]), FW.values(gs[6])
    for k in range(7):
        assert sums[0, 1, k] == f(f(a[k] + b[k]) + c[k]) and sums[1, 1, k] == f(a[k] + c[k])
        assert sums[0, 0, k] == FW.values(gs[4])[k] and sums[0, 2, k] == 0
    rows = FW.result(sums, cnt, skipped)
    assert rows[2]['stitch'] == {k: None for k in FW.KEYS} and rows[2]['stitch_corr']['full_loss'] is None
    assert rows[1]['stitch']['edge_pair_class_acc'] == sums[0, 1, 2] / f(3)
    assert rows[0]['skipped'] == {'bad_rotation': 1, 'no_stitches': 0, 'no_pairs': 0, 'wrong_panel_count': 0}
    assert records.shape == (7, 10) and records[1].tolist() == [0, 0, 0.7, 7, 3, 1, 1, 2, 1, 2] and records[2, 0] == 2
    # the order matters in float32
    big = [_g(counts=(1, 1, 0, 0, 0, 0), loss_sum=2.0 ** 24), _g(counts=(1, 1, 0, 0, 0, 0), loss_sum=1.0),
           _g(counts=(1, 1, 0, 0, 0, 0), loss_sum=1.0)]
    assert FW.fold(big)[0][0, 0, 0] == f(2 ** 24) and FW.fold(big[::-1])[0][0, 0, 0] == f(2 ** 24 + 2)


def test_pool_rows():
    gs = [_g(), _g(counts=(7, 3, 1, 1, 2, 1), loss_sum=0.7, gt_panels=5), _g(ns=0), _g(counts=(3, 3, 0, 0, 0, 0), loss_sum=0.1)]
    records = FW.fold(gs)[3]
    totals, loss, ratios = FW.pool(records, np.array([0, 2, 0, 7]), 3)
    assert totals.shape == (4, 2, 8) and loss.shape == (4, 2) and ratios.shape == (4, 2, 6)
    assert totals[0, 0].tolist() == [10, 8, 2, 4, 3, 1, 2, 1] and totals[0, 1].tolist() == totals[0, 0].tolist()
    assert not totals[1].any() and not ratios[1].any() and not loss[1].any()                    # an empty group gives zeros
    assert totals[2, 0].tolist() == [7, 3, 1, 1, 2, 1, 2, 1] and not totals[2, 1].any()          # counted, not corr
    assert totals[3, 0].tolist() == [20, 14, 3, 5, 5, 2, 6, 3] and totals[3, 1, 7] == 2          # the id 7 counts in the last row only
    assert loss[3, 0] == (5.0 + 0.7) + 0.1 and loss[3, 1] == 5.0 + 0.1
    f = np.float32
    assert ratios[3, 0].tolist() == [f(loss[3, 0] / 20), f(14) / f(20), f(3) / f(5), f(3) / f(5), f(2) / f(6), f(2) / f(5)]


# ---- (3) the chain ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case():
    """the 6 garments of pattern_decode_given.pt and two hand-made ones (given stitches all (0, 0); one non-empty panel) ->
    (preds, gt, data_config, classifier state dict, statistics, restated garments, detail).  Shared with the GPU tests."""
    fx = _load('pattern_decode_given.pt')
    known, full = _load('stitch_pairs_known_answer.pt'), _load('stitch_pairs_full.pt')
    stats = {'f_shift': full['f_shift'], 'f_scale': full['f_scale']}
    dc = fx['data_config']
    preds = {k: torch.cat([v, v[:2].clone()]) for k, v in fx['preds'].items()}
    stitches = torch.cat([fx['stitches'], fx['stitches'][:2].clone()])
    stitches[6] = 0                                                            # no stitch given: state 2
    st = dc['standardize']
    pad = -torch.tensor(st['gt_shift']['outlines'], dtype=torch.float64) / torch.tensor(st['gt_scale']['outlines'], dtype=torch.float64)
    preds['outlines'][7, 1:] = pad.float()                                     # panels 1 .. become padding: one panel, no pair: state 3
    stitches[7] = 0
    stitches[7, 0, 0], stitches[7, 1, 0] = 0, 1                                # one stitch inside the panel that is left
    import pattern_decode_restate as D
    n_panels = D.restate(preds, st, False, stitches=stitches)[0]['num_panels']
    gt_panels = torch.from_numpy(n_panels.copy()).long()
    gt_panels[1] += 1                                                          # garments 1 and 4 have the wrong number of panels
    gt_panels[4] -= 1
    gt = {'stitches': stitches, 'num_panels': gt_panels}
    garments, detail = FW.chain(preds, st, gt, known['state_dict'], stats['f_shift'], stats['f_scale'])
    return preds, gt, dc, known, stats, garments, detail


def test_chain_restatement_on_the_given_stitches_fixture():
    preds, gt, dc, known, stats, garments, detail = chain_case()
    assert preds['outlines'].shape[:3] == (8, 23, 14)
    assert [d['n_labels'] for d in detail[:6]] == [1, 23, 22, 3, 11, 12]
    assert sum(g['first_invalid'] >= 0 for g in garments[:6]) == 2             # two garments are cut at first_invalid
    assert all(g['num_panels'] >= 3 for g in garments[:6])
    assert [FW.state(g) for g in garments] == [0, 0, 0, 0, 0, 0, FW.NO_STITCHES, FW.NO_PAIRS]
    assert garments[7]['num_panels'] == 1 and garments[7]['counts'][0] == 0 and detail[7]['n_labels'] == 1
    assert [FW.corr(g) for g in garments] == [True, False, True, True, False, True, True, True]
    assert all(g['counts'][0] > 0 for g in garments[:6])
    assert sum(g['counts'][4] > 0 for g in garments[:6]) >= 4 and sum(g['counts'][3] > 0 for g in garments[:6]) >= 4
    # a zero denominator inside the counted set: garment 0 has one label, which no enumerated pair carries
    assert garments[0]['counts'][4] == 0 and FW.values(garments[0])[4] == 0
    sums, cnt, skipped, records = FW.fold(garments)
    assert cnt.tolist() == [[6], [4]] and skipped.tolist() == [[0, 1, 1, 2]]
    res = FW.result(sums, cnt, skipped)[0]
    assert all(v is not None and np.isfinite(v) for v in res['stitch'].values())
    totals = FW.pool(records)[0]
    assert totals[0, 0, 7] == 6 and totals[0, 1, 7] == 4 and totals[0, 0, 0] == sum(g['counts'][0] for g in garments[:6])


# ---- (4) the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_framework_header_is_bound_and_exported():
    fw = _lib.parse_header(_lib.FRAMEWORK_HEADER_PATH)
    others = {}
    for h in _lib.HEADERS + _lib.FEATURE_HEADERS + _lib.EVAL_HEADERS + _lib.PLACE_HEADERS:
        others.update(_lib.parse_header(h))
    assert set(fw) == set(SYMBOLS) and not set(fw) & set(others)
    assert _lib.FRAMEWORK_HEADERS == (_lib.FRAMEWORK_HEADER_PATH,)
    assert fw['gpe_framework_eval_add'] == ('i', ['p'] * 9 + ['i', 'i'] + ['p'] * 5 + ['i', 'p', 'p'])
    assert fw['gpe_framework_eval_pool'] == ('i', ['p', 'p', 'l', 'i', 'p', 'p', 'p', 'p'])
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), 'libgpe_hip.so does not export %s' % name
    l = _lib.lib()
    assert l.gpe_abi_version() == 7
    for name, (res, args) in fw.items():
        fn = getattr(l, name)
        assert fn.restype is _lib._CT[res] and list(fn.argtypes) == [_lib._CT[a] for a in args], name
    here = os.path.dirname(os.path.abspath(gpe_amd.__file__))
    assert 'gpe_hip_framework.h' in open(os.path.join(here, 'csrc', 'gpe_common.h')).read()
    assert 'gpe_hip_framework.h' in open(os.path.join(here, 'build.py')).read()


def test_a_framework_symbol_that_is_not_exported_fails_loudly(tmp_path, monkeypatch):
    h = tmp_path / 'framework.h'
    h.write_text('int gpe_framework_not_in_the_library(const double* x, void* stream);\n')
    monkeypatch.setattr(_lib, 'FRAMEWORK_HEADERS', (_lib.FRAMEWORK_HEADER_PATH, str(h)))
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(AttributeError, match='gpe_framework_not_in_the_library'):
        _lib.lib()


def test_bad_arguments_are_rejected_without_a_gpu():
    """The non-NULL 'device' pointers are made-up addresses: an entry point that refuses its arguments never touches them."""
    l = _lib.lib()
    A = 0x7f0000001000
    pointers = ('counts', 'loss_sum', 'num_selected', 'num_stitches', 'first_invalid', 'num_panels', 'gt_num_panels', 'num_edges',
                'place_flags', 'sum', 'cnt', 'skipped', 'records', 'slot', 'status')

    def add(**k):
        d = dict({p: A for p in pointers}, B=4, P=23, slots=2)
        d.update(k)
        return l.gpe_framework_eval_add(*[d[p] for p in pointers[:9]], d['B'], d['P'], *[d[p] for p in pointers[9:14]], d['slots'],
                                        d['status'], None)

    for bad in [dict(P=0), dict(P=65), dict(P=-1), dict(slots=0), dict(slots=-2), dict(B=0), dict(B=-3)] + [{p: None} for p in pointers]:
        assert add(**bad) == -22, bad

    def pool(**k):
        d = dict(table=A, group=A, G=100, n_groups=3, totals=A, loss=A, ratios=A)
        d.update(k)
        return l.gpe_framework_eval_pool(d['table'], d['group'], d['G'], d['n_groups'], d['totals'], d['loss'], d['ratios'], None)

    for bad in (dict(n_groups=-1), dict(n_groups=65536), dict(G=0), dict(G=-5), dict(G=2 ** 31), dict(table=None), dict(totals=None),
                dict(loss=None), dict(ratios=None), dict(group=None)):
        assert pool(**bad) == -22, bad


# ---- (5) the Python refusals ------------------------------------------------------------------------------------------------------------
def test_names_agree_with_the_restatement():
    assert ops.FRAMEWORK_EVAL_KEYS == FW.KEYS and ops.FRAMEWORK_SKIP_REASONS == FW.SKIP_REASONS and ops.FRAMEWORK_SETS == FW.SETS
    assert ops.FRAMEWORK_RECORD == FW.RECORD and ops.FRAMEWORK_TOTALS == FW.TOTALS and ops.STITCH_EVAL_METRICS == FW.METRICS
    assert gpe_amd.evaluation is evaluation and callable(evaluation.eval_framework)


def test_accumulator_checks_need_no_device():
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match='slots'):
            ops.FrameworkAccumulator(slots=bad, total=4, device='cuda')
    for bad in (0, -1, 2.0, True, 2 ** 31):
        with pytest.raises(ValueError, match='total'):
            ops.FrameworkAccumulator(slots=1, total=bad, device='cuda')
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.FrameworkAccumulator(slots=1, total=4, device='cpu')


def _models():
    fx = _load('full3d_small.pt')
    import copy
    torch.manual_seed(fx['seed'])
    model = getattr(gpe_amd.nets, fx['model'])(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(fx['loss_config']))
    known, full = _load('stitch_pairs_known_answer.pt'), _load('stitch_pairs_full.pt')
    stitch = gpe_amd.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    return fx, model.eval(), stitch.eval(), {'f_shift': full['f_shift'], 'f_scale': full['f_scale']}


def test_evaluator_refusals_need_no_device():
    fx, model, stitch, stats = _models()
    dc = fx['data_config']
    FE = evaluation.FrameworkEvaluator
    with pytest.raises(ValueError, match='unknown labels'):
        FE(model, stitch, dc, stats, labels='predicted')
    with pytest.raises(ValueError, match='unknown route'):
        FE(model, stitch, dc, stats, route='dense')
    with pytest.raises(ValueError, match='unknown stitch_route'):
        FE(model, stitch, dc, stats, stitch_route='dense')
    with pytest.raises(TypeError, match='ComposedPatternLoss'):
        FE(stitch, stitch, dc, stats)
    with pytest.raises(TypeError, match='edge-pair classifier'):
        FE(model, model, dc, stats)
    with pytest.raises(ValueError, match='f_scale'):
        FE(model, stitch, dc, {'f_shift': stats['f_shift']})
    ev = FE(model, stitch, dc, stats)
    assert ev.shape is not None and FE(model, stitch, dc, stats, shape_metrics=False).shape is None
    batch = [(fx['features'], {'num_panels': torch.zeros(len(fx['features']), dtype=torch.long)})]
    # the models live on the CPU: there is no CPU path, in Evaluator's wording
    with pytest.raises(RuntimeError, match='no CPU path'):
        ev.run(batch, total=len(fx['features']))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ev.begin(4)
    with pytest.raises(RuntimeError, match='call begin'):
        ev.add_predictions({}, {})
    for m in (model, stitch):
        m.train()
        with pytest.raises(RuntimeError, match=r'call \.eval\(\) first'):
            ev.run(batch, total=1)
        m.eval()
    with pytest.raises(ValueError, match="no 'stitches'"):
        ev._check_gt({'num_panels': 0})
    with pytest.raises(ValueError, match="no 'num_panels'"):
        ev._check_gt({'stitches': 0})
    with pytest.raises(ValueError, match='must be a dict'):
        ev._check_gt(None)
    FE(model, stitch, dc, stats, labels='tags')._check_gt({'num_panels': 0})              # the tag pairing needs no given stitches


def test_label_stitches_is_a_where_on_the_decodes_tensors():
    t = {'edge_slot': torch.zeros(3, 2, 4, dtype=torch.int32), 'stitches': torch.arange(24, dtype=torch.int32).view(3, 2, 4),
         'num_stitches': torch.tensor([4, 0, 3], dtype=torch.int32), 'first_invalid': torch.tensor([-1, -1, 0], dtype=torch.int32)}
    st, n = patterns.DecodedPatterns(t).label_stitches()
    assert st is t['stitches'] and n.dtype == torch.int32 and n.tolist() == [4, 0, 0]
