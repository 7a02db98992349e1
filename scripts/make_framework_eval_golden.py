#!/usr/bin/env python3
"""Generates tests/golden/framework_eval_small.pt: what the REFERENCE'S OWN `_eval_metrics_per_loader`
(nn/metrics/eval_utils.py:35-76), called unmodified, returns for the garments of tests/golden/stitch_eval_<tag>.pt evaluated one
garment per batch — the fold that step 3 of nn/evaluation_scripts/on_test_set.py -st ... -corr performs over the predicted patterns.

  * the loader is a stand-in: a list of one-garment batches {'features': the garment's stored reference logits (`ref_logits` of
    tests/golden/stitch_pairs_<tag>.pt), 'ground_truth': its stored label mask (`ref_mask` of stitch_eval_<tag>.pt), 'name'};
  * the "model" is the identity, so the loss sees the reference's logits as its own model produced them;
  * the loss is the reference's ComposedLoss in the default StitchOnEdge3DPairs configuration (the one the reference's model
    builds: scripts/make_stitch_pairs_golden.py reference_model);
  * the dict is recorded once for all garments ('all') and once for a subset marked "correct" ('corr': every other garment, the
    reference's filter_correct_n_panels pass sees a shorter list and folds it in the same way).

The garment without a stitch (`none`) is left out, by the rule of GarmentStitchPairsDataset._clean_datapoint_list
(nn/data/datasets.py:1149, `if not len(pattern.pattern['stitches']): continue`): that one line is RESTATED here (`if not
len(fx['plants'])`), since the reference reads it from specification files on disk; everything else is the reference's code.

Only runnable where the reference checkout exists.  The new file holds data only; the existing fixtures are read, not rewritten.

    python scripts/make_framework_eval_golden.py [REFERENCE_DIR]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_stitch_pairs_golden as G  # noqa: E402  (sets sys.path onto the stubs and the reference)
from metrics.eval_utils import _eval_metrics_per_loader  # noqa: E402  (the reference's function)

TAGS = ('small', 'gaps', 'none', 'one', 'claimed', 'full')


def _plain(d):
    """the returned dict as data: the value as a Python float (exact for a float32 or float64) and the name of its type"""
    return ({k: (None if v is None else float(v)) for k, v in d.items()},
            {k: (type(v).__name__ + (':' + str(v.dtype) if hasattr(v, 'dtype') else '')) for k, v in d.items()})


if __name__ == '__main__':
    model, known, stats = G.reference_model()
    batches, tags, left_out = [], [], []
    for tag in TAGS:
        pairs = torch.load(os.path.join(G.GOLDEN, 'stitch_pairs_%s.pt' % tag), weights_only=False)
        ev = torch.load(os.path.join(G.GOLDEN, 'stitch_eval_%s.pt' % tag), weights_only=False)
        if not len(ev['plants']):           # datasets.py:1149, restated
            left_out.append(tag)
            continue
        batches.append({'features': pairs['ref_logits'].clone(), 'ground_truth': ev['ref_mask'].clone(), 'name': [tag]})
        tags.append(tag)
    identity = lambda x: x  # noqa: E731
    correct = [i % 2 == 0 for i in range(len(tags))]
    with torch.no_grad():
        ref_all = _eval_metrics_per_loader(identity, model.loss, list(batches), torch.device('cpu'))
        ref_corr = _eval_metrics_per_loader(identity, model.loss, [b for b, c in zip(batches, correct) if c], torch.device('cpu'))
    out = {'tags': tags, 'left_out': left_out, 'correct': correct,
           'loss_config': {k: list(v) if isinstance(v, (list, tuple)) else v for k, v in model.loss.config.items()}}
    out['ref_all'], out['ref_all_types'] = _plain(ref_all)
    out['ref_corr'], out['ref_corr_types'] = _plain(ref_corr)
    out['numpy'], out['torch'] = np.__version__, torch.__version__
    dst = os.path.join(G.GOLDEN, 'framework_eval_small.pt')
    torch.save(out, dst)
    print('framework_eval_small: garments %s (left out: %s), correct %s' % (tags, left_out, correct))
    for name in ('ref_all', 'ref_corr'):
        print('  %-8s %s' % (name, '  '.join('%s=%.9g' % kv for kv in out[name].items())))
    print('  types    %s' % out['ref_all_types'])
    print('  %.1f KB' % (os.path.getsize(dst) / 1024))
