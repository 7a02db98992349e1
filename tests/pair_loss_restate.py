"""fp64 restatement of the training loss of the edge-pair classifier on a batch of pair rows — the reference's ComposedLoss
(nn/metrics/composed_loss.py:83-126) as StitchOnEdge3DPairs calls it — as plain numpy: the specification ops.pair_class_loss and the
device path of metrics.ComposedLoss are tested against (tests/test_gpu_pair_loss.py), pinned to torch's float64 evaluation and to
the reference's recorded numbers by tests/test_pair_loss_host.py.

  loss      mean of max(x, 0) - x y + log1p(exp(-|x|)); for y in {0, 1} this is relu(-x if y else x) + log1p(exp(-|x|))
  class     x > 0 (= round(sigmoid(x)) == 1 for every x the tests use: exactly 0, or at least 1e-5 away from it)
  counts    rows, correct (class == y), true positives, predicted positives, ground-truth positives (y == 1)
  ratios    float32 quotients of the counts, as the reference forms them from float32 tensors; 0 on an empty denominator
  gradient  d loss / d x_i = (sigmoid(x_i) - y_i) / M
"""
import numpy as np

COUNTS = ('pairs', 'correct', 'true_positives', 'predicted_positives', 'gt_positives')
METRICS = ('edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall')


def bce_terms(x, y):
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    """cancellation-free on both sides"""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ratio32(num, den):
    """composed_loss.py:103,123-124 on float32 tensors; 0 on an empty denominator"""
    return np.float32(num) / np.float32(den) if den else np.float32(0)


def evaluate(x, y):
    """-> {'loss' (fp64; nan for no rows), 'counts' {name: int}, 'metrics' {name: value; the ratios float32}, 'grad' fp64 [M]}"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    assert x.shape == y.shape
    M = x.size
    pred = x > 0
    lab = y == 1.0
    counts = {'pairs': M, 'correct': int((pred.astype(np.float64) == y).sum()), 'true_positives': int((pred & lab).sum()),
              'predicted_positives': int(pred.sum()), 'gt_positives': int(lab.sum())}
    loss = float(bce_terms(x, y).sum() / M) if M else float('nan')
    metrics = {'edge_pair_class_loss': loss, 'edge_pair_class_acc': ratio32(counts['correct'], M),
               'stitch_precision': ratio32(counts['true_positives'], counts['predicted_positives']),
               'stitch_recall': ratio32(counts['true_positives'], counts['gt_positives'])}
    return {'loss': loss, 'counts': counts, 'metrics': metrics, 'grad': (sigmoid(x) - y) / M if M else np.zeros(0)}


def reference_arithmetic_bound(x):
    """how far the reference's float32 BCEWithLogitsLoss may lie from the exact mean: 2^-23 mean(|x| + 2)
    (tests/stitch_eval_restate.py reference_arithmetic_bound derives it per term)"""
    x = np.abs(np.asarray(x, dtype=np.float64).reshape(-1))
    return float((2.0 ** -23 * (x + 2.0)).mean()) if x.size else float('inf')
