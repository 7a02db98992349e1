#!/usr/bin/env python3
"""Generates tests/golden/pattern_decode_*.pt: what the REFERENCE'S OWN prediction-to-pattern step makes of a batch of predictions —
Garment3DPatternFullDataset.tags_to_stitches (nn/data/datasets.py:917-968) and NNSewingPattern.pattern_from_tensors /
panel_from_numeric / _edge_dict (nn/data/pattern_converter.py:118-187, 228-271, 510-515), called unbound and unmodified in the
order of Garment3DPatternFullDataset._pred_to_pattern (nn/data/datasets.py:731-767): un-standardise with numpy, recover the stitches,
build the pattern, catch InvalidPatternDefError.

The stand-in object supplies what those functions read: `name`, `properties`, `pattern`, `panel_classifier = None` and a no-op
_invalidate_all_values.  panel_translations = None (turning the predicted universal translation into a panel translation needs the
reference's `pattern` package, which the stubs only name); rotations are real.

Only runnable where the reference checkout exists (like scripts/make_quality_golden.py, whose sys.path set-up on the read-only stubs
it shares).  The fixtures hold data only: configs, inputs, the statistics as lists, the resulting `pattern` dict per garment and
whether InvalidPatternDefError was raised.  Seeded: a re-run writes the same files.

Inputs: quality_restate.make_batch (garment-shaped, with its deliberate faults) plus the faults of pattern_decode_restate.plant_fault;
redrawn until every decision margin of tests/pattern_decode_restate.py is >= quality_restate.MARGIN, so that the reference's fp64
distances and the kernel's fp32 distances decide alike.

    python scripts/make_pattern_decode_golden.py [REFERENCE_DIR]
"""
import copy
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO, os.path.join(REPO, 'tests')]

from data.datasets import Garment3DPatternFullDataset  # noqa: E402  (the reference's class)
from data.pattern_converter import NNSewingPattern, InvalidPatternDefError  # noqa: E402  (the reference's class)
import quality_restate  # noqa: E402
import pattern_decode_restate as R  # noqa: E402

torch.set_num_threads(1)
LSTM = 'models/baseline/lstm_stitch_tags.yaml'
SHIPPED = json.load(open(os.path.join(REPO, 'tests', 'golden', 'shipped_yaml_configs.json')))


class StandIn:
    """what the reference's functions read from a pattern, and the functions themselves, unmodified"""
    pattern_from_tensors = NNSewingPattern.pattern_from_tensors
    panel_from_numeric = NNSewingPattern.panel_from_numeric
    _edge_dict = NNSewingPattern._edge_dict

    def __init__(self, name):
        self.name = name
        self.properties = {}
        self.pattern = {}
        self.panel_classifier = None

    def _invalidate_all_values(self):
        pass


def reference_pattern(pred, data_config, name, stitches=None):
    """Garment3DPatternFullDataset._pred_to_pattern's steps on one garment -> (pattern dict, raised)"""
    prediction = {k: v.clone() for k, v in pred.items()}
    gt_shifts, gt_scales = data_config['standardize']['gt_shift'], data_config['standardize']['gt_scale']
    for key in gt_shifts:
        if key == 'stitch_tags' and not data_config['explicit_stitch_tags']:
            continue
        prediction[key] = prediction[key].cpu().numpy() * gt_scales[key] + gt_shifts[key]
    if stitches is None:
        tags = prediction['stitch_tags']
        stitches = Garment3DPatternFullDataset.tags_to_stitches(                             # ---- the reference, unmodified ----
            torch.from_numpy(tags) if isinstance(tags, np.ndarray) else tags, prediction['free_edges_mask'])
    obj, raised = StandIn(name), False
    try:
        obj.pattern_from_tensors(prediction['outlines'], panel_rotations=prediction['rotations'], panel_translations=None,
                                 stitches=stitches, padded=True)                             # ---- the reference, unmodified ----
    except InvalidPatternDefError:
        raised = True
    assert prediction['outlines'].dtype == np.float64
    return obj.pattern, raised


def run(tag, B, seed, kinds, faults, explicit=False, given=False):
    data_config = copy.deepcopy(SHIPPED[LSTM]['dataset'])
    data_config['max_pattern_len'] = 23                 # nn/data/datasets.py:377-379 with panel_classes_condenced.json
    data_config['explicit_stitch_tags'] = explicit
    P, L, S = data_config['max_pattern_len'], data_config['max_panel_len'], data_config['max_num_stitches']
    stats = data_config['standardize']
    rng = np.random.default_rng(seed)
    for attempt in range(200):
        preds, gt = quality_restate.make_batch(rng, B, P, L, S, data_config, kinds)
        if explicit:                                    # predictions of standardised tags
            sh, sc = (torch.tensor(stats[k]['stitch_tags'], dtype=torch.float32) for k in ('gt_shift', 'gt_scale'))
            preds['stitch_tags'] = (preds['stitch_tags'] * 20 - sh) / sc
        for b in range(B):
            R.plant_fault(rng, preds, b, faults[b % len(faults)], stats)
        st = None
        if given:                                       # the ground truth's stitches, zero padded; one names an empty panel
            st = gt['stitches'].clone()
            st[0, 1, 1] = (P - 1) * L + 2
        _, margin = R.restate(preds, stats, explicit, stitches=st)
        if margin >= quality_restate.MARGIN:
            break
    else:
        raise RuntimeError('%s: no draw with decision margins >= %g' % (tag, quality_restate.MARGIN))
    patterns, raised = [], []
    for b in range(B):
        pat, r = reference_pattern({k: v[b] for k, v in preds.items()}, data_config, 'garment_%d' % b, None if st is None else st[b])
        patterns.append(pat)
        raised.append(r)
    fx = {'data_config': data_config, 'seed': seed, 'draws': attempt + 1, 'margin': margin, 'preds': preds, 'stitches': st,
          'patterns': patterns, 'raised': raised}
    out = os.path.join(REPO, 'tests', 'golden', 'pattern_decode_%s.pt' % tag)
    torch.save(fx, out)
    print('pattern_decode_%-9s B=%-3d draws=%-3d margin=%.2e raised=%s panels=%s stitches=%s  %.0f KB'
          % (tag, B, attempt + 1, margin, ''.join('x' if r else '.' for r in raised), [len(p['panel_order']) for p in patterns],
             [len(p['stitches']) for p in patterns], os.path.getsize(out) / 1024))


if __name__ == '__main__':
    mixed = ['ok', 'pad_real', 'ok', 'open', 'extra', 'free0', 'ok', 'free1', 'odd', 'nost']
    faults = ['none', 'mid_drop', 'empty_stitch', 'none', 'two_rows', 'none', 'dropped_stitch', 'none', 'empty_stitch', 'mid_drop']
    run('lstm', 10, 8001, mixed, faults)
    run('explicit', 6, 8002, ['ok', 'odd', 'open', 'ok', 'extra', 'pad_real'], ['mid_drop', 'none', 'empty_stitch', 'two_rows'],
        explicit=True)
    run('given', 6, 8003, ['ok', 'open', 'ok', 'pad_real'], ['none', 'none', 'mid_drop', 'two_rows'], given=True)
