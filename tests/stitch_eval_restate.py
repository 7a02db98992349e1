"""fp64 restatement of the evaluation of the edge-pair classifier over ALL edge pairs of a garment against ground-truth stitches —
what the reference computes with the labels of NNSewingPattern.all_edge_pairs (nn/data/pattern_converter.py:458-499) and
ComposedLoss (nn/metrics/composed_loss.py:83-126) — as plain numpy / python on top of tests/stitch_pairs_restate.py: the
specification ops.stitch_pairs_eval is tested against (tests/test_gpu_stitch_eval.py), pinned to the reference's recorded numbers
by tests/test_stitch_eval_host.py.

A pair is (i, j, r, c) as in stitch_pairs_restate; a ground-truth stitch is ((panel, edge), (panel, edge)) in either orientation.

reference_arithmetic: the reference's loss is torch's float32 BCEWithLogitsLoss, which evaluates a term as
(1 - y) * x - log_sigmoid(x) in float32.  The subtraction cancels: a term carries up to half a float32 ulp OF |x| (4.8e-7 at
8 <= |x| < 16) whatever its own size, and over a garment's pairs this does not average out (3e-7 on the mean of every fixture).
True transcribes that arithmetic and must reproduce the reference's recorded loss (tests/test_stitch_eval_host.py); False is the
exact fp64 term = this build's specification, which the kernels evaluate as relu(-+x) + log1p(exp(-|x|)) without cancellation.
"""
import numpy as np

import stitch_pairs_restate as R

COUNTS = ('pairs', 'correct', 'true_positives', 'predicted_positives', 'gt_positives', 'selected_tp')


def stitch_set(stitches):
    """_stitches_as_set (:501-508): ordered tuples, as given"""
    return {((int(a[0]), int(a[1])), (int(b[0]), int(b[1]))) for a, b in stitches}


def labels(pairs, stitches):
    """the mask of all_edge_pairs (:492): pair_id in stitch_set or the reversed pair_id in stitch_set"""
    st = stitch_set(stitches)
    return np.asarray([(((i, r), (j, c)) in st) or (((j, c), (i, r)) in st) for i, j, r, c in pairs], dtype=bool)


def stitches_from_ids(ids, num, L):
    """the product's ground-truth layout (edge ids panel * L + edge, [2, S] with a count) -> stitch tuples; ids outside
    0 .. E - 1 are kept as they are: no pair matches them"""
    a, b = np.asarray(ids)[0][:num], np.asarray(ids)[1][:num]
    return [((int(x) // L, int(x) % L), (int(y) // L, int(y) % L)) for x, y in zip(a, b)]


def bce_terms(logits, y, reference_arithmetic=False):
    """BCEWithLogitsLoss per element in fp64: relu(-x if y else x) + log1p(exp(-|x|)); reference_arithmetic: the float32 terms
    (1 - y) * x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|)), every operation rounded to float32"""
    if reference_arithmetic:
        x = np.asarray(logits, dtype=np.float32)
        log_sigmoid = (np.minimum(x, np.float32(0)) - np.log1p(np.exp(-np.abs(x)))).astype(np.float32)
        return ((np.float32(1) - np.asarray(y, dtype=np.float32)) * x - log_sigmoid).astype(np.float32).astype(np.float64)
    x = np.asarray(logits, dtype=np.float64)
    return np.maximum(np.where(y, -x, x), 0.0) + np.log1p(np.exp(-np.abs(x)))


def reference_arithmetic_bound(logits):
    """how far the mean of the float32 terms may lie from the mean of the exact ones.  Per term: log_sigmoid(x) and the final
    difference are each rounded at a magnitude <= |x| + log 2, i.e. by at most 2^-24 (|x| + log 2) each; exp, log1p and their
    difference inside log_sigmoid act on numbers <= log 2 and add less than 3 * 2^-24 * log 2.  Together < 2^-23 (|x| + 2).
    inf for no pair"""
    x = np.abs(np.asarray(logits, dtype=np.float64))
    return float((2.0 ** -23 * (x + 2.0)).mean()) if len(x) else float('inf')


def _ratio(num, den):
    """composed_loss.py:123-124: 0 on an empty denominator"""
    return float(num) / float(den) if den else 0.0


def evaluate(pairs, logits, stitches, reference_arithmetic=False):
    """-> {'mask', 'loss_sum', 'counts' {name: int}}: class rule = R.positives; selected_tp = the survivors of the selection
    (R.stitches, intended indexing) whose pair is labelled"""
    y = labels(pairs, stitches)
    lg = np.asarray(logits)
    pred = np.zeros(len(pairs), dtype=bool)
    pred[R.positives(lg)] = True
    sel = {s[0] for s in R.stitches(pairs, lg)}
    counts = {'pairs': len(pairs), 'correct': int((pred == y).sum()), 'true_positives': int((pred & y).sum()),
              'predicted_positives': int(pred.sum()), 'gt_positives': int(y.sum()),
              'selected_tp': int(sum(1 for k, p in enumerate(pairs) if y[k] and tuple(p) in sel)), 'selected': len(sel)}
    return {'mask': y, 'loss_sum': float(bce_terms(lg, y, reference_arithmetic).sum()) if len(pairs) else 0.0, 'counts': counts}


def pooled(results):
    """the call's metrics from the per-garment results: the loss is the mean over the concatenated pairs"""
    t = {k: sum(r['counts'][k] for r in results) for k in COUNTS + ('selected',)}
    return {'edge_pair_class_loss': _ratio(sum(r['loss_sum'] for r in results), t['pairs']),
            'edge_pair_class_acc': _ratio(t['correct'], t['pairs']),
            'stitch_precision': _ratio(t['true_positives'], t['predicted_positives']),
            'stitch_recall': _ratio(t['true_positives'], t['gt_positives']),
            'selected_precision': _ratio(t['selected_tp'], t['selected']),
            'selected_recall': _ratio(t['selected_tp'], t['gt_positives'])}
