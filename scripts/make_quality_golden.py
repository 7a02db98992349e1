#!/usr/bin/env python3
"""Generates tests/golden/quality_*.pt: the quality metrics of the REFERENCE'S OWN ComposedPatternLoss
(nn/metrics/composed_loss.py:268-277,365-424 with nn/metrics/metrics.py and nn/data/datasets.py tags_to_stitches), called under
no_grad with with_quality_eval = True on garment-shaped inputs.

Only runnable where the reference checkout exists (like oracle/refgen/make_golden.py, whose stubs it puts on sys.path read-only).
The fixtures hold data only: configs, inputs, the matched ground truth and the reference's loss dict with None kept as None.
Seeded: a re-run writes the same files.

Inputs are shaped like real garments, or the metrics would be trivial: closed edge loops in cm (standardised, padded with the
pad vector, empty panels at the end), predictions = ground truth + noise with deliberate faults (padding rows made real, loops
opened by > 3 cm, an extra panel, whole batches without a correct pattern), stitch tags as well-separated 3-D points shared by
both sides of a stitch, free-edge logits of both signs with some flipped.  Every decision of the metrics keeps a relative
margin >= 1e-4 from its bound (tests/quality_restate.py); a pattern that misses it is redrawn.

    python scripts/make_quality_golden.py [REFERENCE_DIR]
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

from metrics.composed_loss import ComposedPatternLoss  # noqa: E402  (the reference's class)
import quality_restate  # noqa: E402

torch.set_num_threads(1)
LSTM, ATT = 'models/baseline/lstm_stitch_tags.yaml', 'models/att/att.yaml'
SHIPPED = json.load(open(os.path.join(REPO, 'tests', 'golden', 'shipped_yaml_configs.json')))


def configs(yaml_rel):
    data_config = copy.deepcopy(SHIPPED[yaml_rel]['dataset'])
    data_config['max_pattern_len'] = 23                 # nn/data/datasets.py:377-379 with panel_classes_condenced.json
    return data_config, copy.deepcopy(SHIPPED[yaml_rel]['NN']['loss'])


def _matched_gt(loss, preds, gt, epoch):
    """the ground truth the reference evaluates its metrics on (gt_rotated), with the reference's own helpers"""
    with torch.no_grad():
        loss.epoch, loss.device = epoch, preds['outlines'].device
        g = {k: v.clone() for k, v in gt.items()}
        if loss.config['panel_order_inariant_loss']:
            g = loss._gt_order_match(preds, g)
        ne = g['num_edges'].int().view(-1)
        if loss.config['panel_origin_invariant_loss']:
            g = loss._rotate_gt(preds, g, ne, epoch)
    return g


def run(tag, yaml_rel, B, seed, epoch, kinds, loss_override=None, explicit=False, permute=False, all_stitches=False):
    data_config, loss_cfg = configs(yaml_rel)
    data_config['explicit_stitch_tags'] = explicit
    if loss_override:
        loss_cfg.update(loss_override)
    P, L = data_config['max_pattern_len'], data_config['max_panel_len']
    S = data_config['max_num_stitches']
    rng = np.random.default_rng(seed)
    for attempt in range(200):
        preds, gt = quality_restate.make_batch(rng, B, P, L, S, data_config, kinds, all_stitches)
        if permute:
            quality_restate.permute_panels(rng, preds, gt, loss_cfg.get('panel_origin_invariant_loss', False))
        loss = ComposedPatternLoss(data_config, copy.deepcopy(loss_cfg))
        gt_m = _matched_gt(loss, preds, gt, epoch)
        _, margin = quality_restate.restate(loss.q_components, epoch, loss_cfg['epoch_with_stitches'],
                                            data_config['standardize'], explicit, preds, gt_m)
        if margin >= quality_restate.MARGIN:
            break
    else:
        raise RuntimeError('%s: no draw with decision margins >= %g' % (tag, quality_restate.MARGIN))
    loss = ComposedPatternLoss(data_config, copy.deepcopy(loss_cfg))
    loss.with_quality_eval = True
    with torch.no_grad():
        _, loss_dict, _ = loss({k: v.clone() for k, v in preds.items()}, {k: v.clone() for k, v in gt.items()}, epoch=epoch)
    ref = {k: (None if v is None else float(v)) for k, v in loss_dict.items()}
    fx = {'yaml': yaml_rel, 'data_config': data_config, 'loss_config': loss_cfg, 'epoch': epoch, 'seed': seed,
          'draws': attempt + 1, 'margin': margin, 'preds': preds, 'gt': gt, 'gt_matched': gt_m, 'loss_dict': ref,
          'none_keys': sorted(k for k, v in ref.items() if v is None)}
    out = os.path.join(REPO, 'tests', 'golden', 'quality_%s.pt' % tag)
    torch.save(fx, out)
    print('quality_%-22s B=%-3d draws=%-3d margin=%.2e  %s' % (tag, B, attempt + 1, margin,
          ' '.join('%s=%s' % (k, 'None' if v is None else '%.5g' % v) for k, v in ref.items()
                   if k in quality_restate_keys)))


quality_restate_keys = ('num_panels_accuracy', 'corr_num_edges_accuracy', 'corr_panel_shape_l2', 'stitch_precision',
                        'stitch_recall', 'corr_stitch_recall', 'free_edge_acc')

if __name__ == '__main__':
    mixed = ['ok', 'pad_real', 'ok', 'open', 'extra', 'free0', 'ok', 'free1', 'odd', 'nost']
    run('lstm_e40', LSTM, 10, 7001, 40, mixed)
    run('lstm_e0', LSTM, 6, 7002, 0, mixed)
    run('att', ATT, 8, 7003, 0, mixed)
    run('matching', LSTM, 8, 7004, 40, mixed, permute=True,
        loss_override={'panel_order_inariant_loss': True, 'order_by': 'placement', 'panel_origin_invariant_loss': True})
    run('explicit_tags', LSTM, 6, 7005, 40, mixed, explicit=True)
    run('no_correct', LSTM, 4, 7006, 40, ['extra'])
    run('full', LSTM, 32, 7007, 40, ['ok', 'ok', 'odd', 'ok', 'open', 'ok', 'extra', 'ok'], all_stitches=True)
