"""not-gpu: the evaluation of the edge-pair classifier over all edge pairs (ops.stitch_pairs_eval /
StitchOnEdge3DPairs.evaluate_stitches).
  (1) the fp64 restatement (tests/stitch_eval_restate.py) reproduces what the reference's own all_edge_pairs + ComposedLoss recorded
      (tests/golden/stitch_eval_*.pt, scripts/make_stitch_eval_golden.py): the mask and every counter and ratio exactly, the loss
      within 1e-6 relative of the reference's fp32 value in the reference's float32 arithmetic, and the exact fp64 loss within
      that arithmetic's rounding bound;
  (2) the C ABI: the new symbols are declared and exported, -22 on bad arguments without a GPU;
  (3) the host-side refusals, all before any device check;
  (4) the keys of evaluate_stitches' loss_dict follow the model's loss configuration."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import gpe_amd
from gpe_amd import _lib
import stitch_pairs_restate as R
import stitch_eval_restate as EV

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'stitch_eval_*.pt')))
IDS = [os.path.basename(f)[len('stitch_eval_'):-3] for f in FIXTURES]
SYMBOLS = ('gpe_stitch_pairs_labels', 'gpe_stitch_pairs_eval_fwd', 'gpe_stitch_pairs_eval_reduce', 'gpe_stitch_eval_finalize')
# (pairs, ground-truth positives, predicted positives, true positives) of the reference's logits and mask
TABLE = {'claimed': (290, 3, 7, 2), 'gaps': (697, 6, 8, 1), 'small': (209, 4, 9, 1), 'full': (49588, 40, 307, 4),
         'one': (56, 1, 1, 0), 'none': (95, 0, 0, 0)}


def _load(path):
    ev = torch.load(path, weights_only=False)
    fx = torch.load(os.path.join(GOLDEN, 'stitch_pairs_%s.pt' % ev['tag']), weights_only=False)
    fx['pairs'] = [tuple(int(v) for v in row) for row in fx['ref_order'].tolist()]
    return ev, fx


def test_every_garment_fixture_has_its_evaluation():
    assert set(IDS) == set(TABLE)
    orientations = set()
    for path in FIXTURES:
        ev, fx = _load(path)
        c = ev['counts']
        assert (c['pairs'], c['gt_positives'], c['predicted_positives'], c['true_positives']) == TABLE[ev['tag']]
        assert ev['plants'] == fx['plants'] and os.path.getsize(path) < (1 << 20)
        orientations |= {a[0] < b[0] for a, b in ev['plants']}
        assert ev['loss_config']['loss_components'] == ['edge_pair_class']
        assert ev['loss_config']['quality_components'] == ['edge_pair_class', 'edge_pair_stitch_recall']
        assert fx['margin_zero'] >= 4 * fx['tol']           # class decisions are safe in every arithmetic
    assert orientations == {True, False}                    # the reversed lookup of all_edge_pairs is exercised
    one, none = _load(os.path.join(GOLDEN, 'stitch_eval_one.pt'))[0], _load(os.path.join(GOLDEN, 'stitch_eval_none.pt'))[0]
    assert one['ref_loss_dict']['stitch_precision'] == 0 and one['ref_loss_types']['stitch_precision'] == 'Tensor'
    assert none['ref_loss_types']['stitch_precision'] == 'int' and none['ref_loss_types']['stitch_recall'] == 'int'


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_restatement_reproduces_the_reference(path):
    ev, fx = _load(path)
    plants = [(tuple(a), tuple(b)) for a, b in ev['plants']]
    got = EV.evaluate(fx['pairs'], fx['ref_logits'].numpy(), plants)
    assert np.array_equal(got['mask'], ev['ref_mask'].numpy())
    for k, v in ev['counts'].items():
        assert got['counts'][k] == v, k
    m = EV.pooled([got])
    ref = ev['ref_loss_dict']
    assert set(ref) == {'edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall'}
    for k in ('edge_pair_class_acc', 'stitch_precision', 'stitch_recall'):
        assert np.float32(m[k]) == np.float32(ref[k]), k
    assert ref['edge_pair_class_loss'] == ev['ref_full_loss']
    # the product's layout of the same ground truth gives the same labels
    L = fx['edges'].shape[1]
    ids = np.asarray([[a[0] * L + a[1] for a, _ in plants], [b[0] * L + b[1] for _, b in plants]], dtype=np.int64).reshape(2, -1)
    assert np.array_equal(EV.labels(fx['pairs'], EV.stitches_from_ids(ids, len(plants), L)), got['mask'])
    # selected stitches: a subset of the labelled positives
    assert 0 <= got['counts']['selected_tp'] <= min(got['counts']['true_positives'], got['counts']['selected'])


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_restated_loss_is_within_1e6_relative_of_the_references_fp32_value(path):
    """The reference's value is torch's float32 BCEWithLogitsLoss, (1 - y) * x - log_sigmoid(x) per element: the restatement
    reproduces it within 1e-6 relative in its reference arithmetic (measured: 1.1e-7 at worst, `claimed`).  The exact fp64 terms
    = the specification of the kernels cannot: the float32 difference cancels and leaves up to half an ulp of |x| on every term
    (measured against the exact mean: small 4.8e-7, claimed 8.2e-7, one 1.8e-6, gaps 2.5e-6, full 4.8e-6, none 1.7e-3 relative;
    2.9e-7 .. 3.5e-7 absolute each).  So the exact mode is pinned twice: to torch's own float64 evaluation, and to the reference
    arithmetic within the rounding bound of that arithmetic (EV.reference_arithmetic_bound)."""
    ev, fx = _load(path)
    plants = [(tuple(a), tuple(b)) for a, b in ev['plants']]
    logits, ref = fx['ref_logits'].numpy(), ev['ref_loss_dict']['edge_pair_class_loss']
    as_ref = EV.pooled([EV.evaluate(fx['pairs'], logits, plants, reference_arithmetic=True)])['edge_pair_class_loss']
    exact = EV.pooled([EV.evaluate(fx['pairs'], logits, plants)])['edge_pair_class_loss']
    t64 = torch.nn.functional.binary_cross_entropy_with_logits(fx['ref_logits'].double(), ev['ref_mask'].double()).item()
    bound = EV.reference_arithmetic_bound(logits)
    print('%s: reference (float32) %.12g  restated in its arithmetic %.12g (relative %.3g)  exact %.12g  torch float64 %.12g  '
          '|exact - reference| %.3g (rounding bound %.3g)' % (ev['tag'], ref, as_ref, abs(as_ref - ref) / ref, exact, t64,
                                                              abs(exact - ref), bound))
    assert abs(as_ref - ref) <= 1e-6 * ref
    assert abs(exact - t64) <= bound * 2.0 ** -29            # torch's float64 evaluation cancels alike, at float64's ulp
    assert abs(exact - as_ref) <= bound and abs(exact - ref) <= bound + 1e-6 * ref


def test_restatement_conventions():
    pairs = R.enumerate_pairs([2, 0, 2])
    assert pairs == [(0, 2, 0, 0), (0, 2, 0, 1), (0, 2, 1, 0), (0, 2, 1, 1)]
    # reversed orientation, a duplicate, a same-panel entry and an absent panel
    st = [((2, 1), (0, 0)), ((0, 0), (2, 1)), ((0, 0), (0, 1)), ((1, 0), (2, 0))]
    assert EV.labels(pairs, st).tolist() == [False, True, False, False]
    got = EV.evaluate(pairs, np.asarray([-3.0, 2.0, 1.0, -0.5]), st)
    c = got['counts']
    assert (c['pairs'], c['correct'], c['true_positives'], c['predicted_positives'], c['gt_positives']) == (4, 3, 1, 2, 1)
    assert c['selected'] == 2 and c['selected_tp'] == 1
    want = np.log1p(np.exp(-3.0)) + np.log1p(np.exp(-2.0)) + (1.0 + np.log1p(np.exp(-1.0))) + np.log1p(np.exp(-0.5))
    assert abs(got['loss_sum'] - want) < 1e-12
    m = EV.pooled([got, EV.evaluate([], np.zeros(0), [])])
    assert m['edge_pair_class_loss'] == got['loss_sum'] / 4 and m['stitch_precision'] == 0.5 and m['selected_recall'] == 1.0
    empty = EV.pooled([EV.evaluate([], np.zeros(0), [])])
    assert set(empty.values()) == {0.0}


def test_header_declares_and_library_exports_the_symbols():
    sigs = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in sigs and hasattr(raw, name), name
        res, args = sigs[name]
        assert res == 'i' and args[-1] == 'p'
    assert _lib.lib().gpe_abi_version() == 7
    # the evaluating twins take their prediction twins' operands first
    assert sigs['gpe_stitch_pairs_eval_fwd'][1][:14] == sigs['gpe_stitch_pairs_fwd'][1][:14]
    assert sigs['gpe_stitch_pairs_eval_reduce'][1][:11] == sigs['gpe_stitch_pairs_reduce'][1][:11]


def test_bad_arguments_are_rejected_without_a_gpu():
    l = _lib.lib()
    assert l.gpe_stitch_pairs_labels(None, None, 1, 4, 4, 2, None, None) == -22
    assert l.gpe_stitch_pairs_eval_fwd(None, 0, 0, 0, None, None, None, None, None, 1, 4, 4, None, None, None, None, None, None) == -22
    assert l.gpe_stitch_pairs_eval_reduce(None, 1, None, 1, 4, 4, 0, 1, 1, None, None, None, None, None, None) == -22
    assert l.gpe_stitch_eval_finalize(None, 4, 2, None, None, None, None, 1, 4, 4, None, None, None, None) == -22


def _model(loss_config=None):
    known = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    model = gpe_amd.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), dict(loss_config or {}))
    model.load_state_dict(known['state_dict'])
    return model.eval()


def _inputs():
    fx = torch.load(os.path.join(GOLDEN, 'stitch_pairs_small.pt'), weights_only=False)
    stats = {'f_shift': fx['f_shift'], 'f_scale': fx['f_scale']}
    return fx['edges'][None], fx['num_edges'][None], stats


def test_argument_errors_come_before_any_device_check():
    model = _model()
    edges, ne, stats = _inputs()
    gt, n = torch.zeros(1, 2, 3, dtype=torch.int64), torch.tensor([2])
    ok = (edges, ne, model.mlp, stats['f_shift'], stats['f_scale'])
    for bad_gt in (torch.zeros(1, 3, 2, dtype=torch.int64), torch.zeros(2, 2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64),
                   torch.zeros(1, 2, 3), torch.zeros(1, 2, 3, dtype=torch.bool), gt.to('meta')):
        with pytest.raises(ValueError, match='gt_stitches'):
            gpe_amd.ops.stitch_pairs_eval(*ok, bad_gt, n)
    for bad_n in (torch.tensor([2, 2]), torch.tensor([[2]]), torch.tensor([2.0]), n.to('meta')):
        with pytest.raises(ValueError, match='gt_num_stitches'):
            gpe_amd.ops.stitch_pairs_eval(*ok, gt, bad_n)
    with pytest.raises(ValueError, match='unknown route'):
        gpe_amd.ops.stitch_pairs_eval(*ok, gt, n, route='dense')
    with pytest.raises(ValueError, match='num_edges'):
        gpe_amd.ops.stitch_pairs_eval(edges, ne[:, :-1], model.mlp, stats['f_shift'], stats['f_scale'], gt, n)
    # well-formed arguments on the CPU: the product has no CPU path (S = 0 is well-formed)
    for g in (gt, torch.zeros(1, 2, 0, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            gpe_amd.ops.stitch_pairs_eval(*ok, g, n)
    with pytest.raises(RuntimeError, match='no CPU path'):
        model.evaluate_stitches(edges, ne, gt, n, stats)


def test_evaluate_stitches_refuses_training_mode():
    model = _model().train()
    edges, ne, stats = _inputs()
    with pytest.raises(RuntimeError, match='eval'):
        model.evaluate_stitches(edges, ne, torch.zeros(1, 2, 0, dtype=torch.int64), torch.tensor([0]), stats)


@pytest.mark.parametrize('loss_config,quality,want', [
    ({}, True, {'edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall'}),
    ({}, False, {'edge_pair_class_loss'}),
    ({'quality_components': ['edge_pair_class']}, True, {'edge_pair_class_loss', 'edge_pair_class_acc'}),
    ({'quality_components': ['edge_pair_stitch_recall']}, True, {'edge_pair_class_loss', 'stitch_precision', 'stitch_recall'}),
    ({'loss_components': [], 'quality_components': ['edge_pair_class']}, True, {'edge_pair_class_acc'}),
    ({'loss_components': [], 'quality_components': []}, True, set()),
])
def test_loss_dict_keys_follow_the_loss_configuration(monkeypatch, loss_config, quality, want):
    model = _model(loss_config)
    model.loss.with_quality_eval = quality
    edges, ne, stats = _inputs()
    names = gpe_amd.ops.STITCH_EVAL_METRICS
    seen = {}

    def fake(edges3d, num_edges, mlp, f_shift, f_scale, gt_stitches, gt_num_stitches, **kw):
        seen.update(kw, shift=f_shift)
        return {'metrics': {k: torch.tensor(float(i)) for i, k in enumerate(names)}}

    monkeypatch.setattr(gpe_amd.ops, 'stitch_pairs_eval', fake)
    out, loss_dict = model.evaluate_stitches(edges, ne, torch.zeros(1, 2, 0, dtype=torch.int64), torch.tensor([0]), stats, route='rows')
    assert set(loss_dict) == want and seen['route'] == 'rows' and seen['shift'] == stats['f_shift']
    for k, v in loss_dict.items():
        assert float(v) == names.index(k)
    # the keys are those the loss object itself produces for this configuration
    preds, gt = torch.tensor([2.0, -1.0, 0.5]), torch.tensor([True, False, False])
    assert set(model.loss(preds, gt)[1]) == want
