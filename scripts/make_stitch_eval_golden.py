#!/usr/bin/env python3
"""Generates tests/golden/stitch_eval_<tag>.pt from every garment fixture tests/golden/stitch_pairs_<tag>.pt: what the REFERENCE'S
OWN evaluation of the edge-pair classifier over all edge pairs returns against ground-truth stitches —

  * pattern['stitches'] is filled from the fixture's planted stitches (`plants`: (source panel, edge) -> (target panel, edge))
    through NNSewingPattern._stitch_entry, each in its own orientation, so some name the later panel first;
  * the label mask is what NNSewingPattern.all_edge_pairs returns (nn/data/pattern_converter.py:458-499, with _stitches_as_set),
    called unbound and unmodified on the stand-in object of scripts/make_stitch_pairs_golden.py;
  * the numbers are what the reference's ComposedLoss (nn/metrics/composed_loss.py) returns on the reference's logits (the
    fixture's `ref_logits`, reproduced here by the reference's model) and that mask, with the default StitchOnEdge3DPairs loss
    configuration: edge_pair_class_loss, edge_pair_class_acc, stitch_precision, stitch_recall.

Only runnable where the reference checkout exists.  The new files hold data only; the existing fixtures are read, not rewritten.

    python scripts/make_stitch_eval_golden.py [REFERENCE_DIR]
"""
import glob
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_stitch_pairs_golden as G  # noqa: E402  (sets sys.path onto the stubs and the reference; defines the stand-in)


def _num(v):
    """the reference returns tensors, or the Python int 0 on an empty denominator"""
    return float(v)


def record(path, model, stats):
    fx = torch.load(path, weights_only=False)
    tag = fx['tag']
    obj = G.StandIn(fx['edges'].numpy(), fx['num_edges'].numpy())
    obj.pattern['stitches'] = [obj._stitch_entry('p%02d' % ps, int(es), 'p%02d' % pt, int(et)) for (ps, es), (pt, et) in fx['plants']]
    with torch.no_grad():
        rows, mapping, mask = obj.all_edge_pairs(device='cpu')
        order = [(G.slot(a[0]), G.slot(b[0]), a[1], b[1]) for a, b in mapping]
        assert order == [tuple(int(v) for v in r) for r in fx['ref_order'].tolist()]
        shift, scale = torch.tensor(stats['f_shift']), torch.tensor(stats['f_scale'])
        logits = model((rows - shift) / scale)
        assert torch.equal(logits.float(), fx['ref_logits']), 'the reference no longer reproduces the stored logits'
        gt = torch.tensor(mask)
        full, loss_dict, _ = model.loss(logits, gt)
    pred = torch.round(torch.sigmoid(logits)).bool()
    out = {'tag': tag, 'plants': fx['plants'], 'ref_mask': gt.clone(),
           'ref_loss_dict': {k: _num(v) for k, v in loss_dict.items()}, 'ref_full_loss': _num(full),
           'ref_loss_types': {k: type(v).__name__ for k, v in loss_dict.items()},
           'loss_config': {k: list(v) if isinstance(v, (list, tuple)) else v for k, v in model.loss.config.items()},
           'counts': {'pairs': int(gt.numel()), 'gt_positives': int(gt.sum()), 'predicted_positives': int(pred.sum()),
                      'true_positives': int((pred & gt).sum()), 'correct': int((pred == gt).sum())}}
    dst = os.path.join(G.GOLDEN, 'stitch_eval_%s.pt' % tag)
    torch.save(out, dst)
    c = out['counts']
    print('stitch_eval_%-8s pairs=%-6d gt+=%-3d pred+=%-4d tp=%-3d  %s  %.1f KB'
          % (tag, c['pairs'], c['gt_positives'], c['predicted_positives'], c['true_positives'],
             '  '.join('%s=%.6g' % kv for kv in out['ref_loss_dict'].items()), os.path.getsize(dst) / 1024))


if __name__ == '__main__':
    model, known, stats = G.reference_model()
    for path in sorted(glob.glob(os.path.join(G.GOLDEN, 'stitch_pairs_*.pt'))):
        if 'known_answer' not in path:
            record(path, model, stats)
