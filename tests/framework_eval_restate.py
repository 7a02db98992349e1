"""A numpy restatement of the two-stage evaluation pass (include/gpe_hip_framework.h, ops.FrameworkAccumulator,
evaluation.FrameworkEvaluator): which garments count (the reference's GarmentStitchPairsDataset._clean_datapoint_list,
nn/data/datasets.py:1134-1159), their per-garment values, and the fold of nn/metrics/eval_utils.py:35-76 with one garment per batch
— np.float32 adds in garment order.  Not a test: a helper of tests/test_framework_eval_host.py and tests/test_gpu_framework_eval.py.

`chain` restates the whole per-garment path from the existing restatements: pattern_decode_restate.restate ->
pattern_place_restate.restate -> stitch_eval_restate.evaluate on the fp64 logits of stitch_pairs_restate.logits64."""
import numpy as np

import pattern_decode_restate as D
import pattern_place_restate as PL
import stitch_eval_restate as EV
import stitch_pairs_restate as R

KEYS = ('full_loss', 'edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall', 'selected_precision',
        'selected_recall')
SETS = ('stitch', 'stitch_corr')
SKIP_REASONS = ('bad_rotation', 'no_stitches', 'no_pairs', 'wrong_panel_count')
COUNTS = EV.COUNTS                                      # pairs, correct, true_positives, predicted_positives, gt_positives, selected_tp
RECORD = ('state', 'corr', 'loss_sum') + COUNTS + ('num_selected',)
TOTALS = COUNTS + ('num_selected', 'garments')
METRICS = KEYS[1:]                                      # the six pooled ratios, in the order of ops.STITCH_EVAL_METRICS
BAD_ROTATION, NO_STITCHES, NO_PAIRS, COUNTED = 1, 2, 3, 0


def garment(counts, loss_sum, num_selected, num_stitches, first_invalid, num_panels, gt_num_panels, num_edges, place_flags, slot=0):
    """one garment as the kernel sees it (counts: the six of COUNTS)"""
    return {'counts': [int(c) for c in counts], 'loss_sum': float(loss_sum), 'num_selected': int(num_selected),
            'num_stitches': int(num_stitches), 'first_invalid': int(first_invalid), 'num_panels': int(num_panels),
            'gt_num_panels': int(gt_num_panels), 'num_edges': [int(n) for n in num_edges], 'place_flags': [int(f) for f in place_flags],
            'slot': int(slot)}


def n_labels(g):
    """the stitches _pred_to_pattern leaves (datasets.py:756-765): those before the first invalid one"""
    return g['first_invalid'] if g['first_invalid'] >= 0 else g['num_stitches']


def state(g):
    """the first rule that matches"""
    if any(f != 0 and n > 0 for f, n in zip(g['place_flags'], g['num_edges'])):
        return BAD_ROTATION                 # the reference's scipy call raises, uncaught: the documented deviation
    if n_labels(g) == 0:
        return NO_STITCHES                  # datasets.py:1149
    if g['counts'][0] == 0:
        return NO_PAIRS                     # all_edge_pairs raises InvalidPatternDefError, eval_utils.py:49 skips the batch
    return COUNTED


def corr(g):
    """datasets.py:1152-1156"""
    return g['num_panels'] == g['gt_num_panels']


def ratio32(num, den):
    """composed_loss.py:123-124: 0 on an empty denominator; otherwise one float32 division of two exact integers"""
    return np.float32(num) / np.float32(den) if den else np.float32(0)


def values(g):
    """the seven float32 values of a counted garment, in the order of KEYS"""
    pairs, correct, tp, pred, gtp, sel_tp = g['counts']
    loss = np.float32(np.float64(g['loss_sum']) / np.float64(pairs))
    return [loss, loss, ratio32(correct, pairs), ratio32(tp, pred), ratio32(tp, gtp), ratio32(sel_tp, g['num_selected']),
            ratio32(sel_tp, gtp)]


def record(g):
    return [float(state(g)), float(corr(g)), g['loss_sum']] + [float(c) for c in g['counts']] + [float(g['num_selected'])]


def fold(garments, slots=1):
    """-> (sums float32 [2, slots, 7], cnt int32 [2, slots], skipped int32 [slots, 4], records float64 [G, 10])"""
    sums = np.zeros((2, slots, len(KEYS)), np.float32)
    cnt = np.zeros((2, slots), np.int32)
    skipped = np.zeros((slots, 4), np.int32)
    for g in garments:
        s, st = g['slot'], state(g)
        if st != COUNTED:
            skipped[s, st - 1] += 1
            continue
        v = values(g)
        for i in ((0, 1) if corr(g) else (0,)):
            for k in range(len(KEYS)):
                sums[i, s, k] = np.float32(sums[i, s, k] + v[k])
            cnt[i, s] += 1
        if not corr(g):
            skipped[s, 3] += 1
    return sums, cnt, skipped, np.asarray([record(g) for g in garments], np.float64).reshape(len(garments), len(RECORD))


def result(sums, cnt, skipped):
    """what FrameworkAccumulator.read returns: per slot {'stitch': {...}, 'stitch_corr': {...}, 'skipped': {...}}"""
    rows = []
    for s in range(cnt.shape[1]):
        row = {name: {k: (np.float32(sums[i, s, j]) / np.float32(cnt[i, s]) if cnt[i, s] else None) for j, k in enumerate(KEYS)}
               for i, name in enumerate(SETS)}
        row['skipped'] = {r: int(skipped[s, j]) for j, r in enumerate(SKIP_REASONS)}
        rows.append(row)
    return rows


def pool(records, groups=None, n_groups=0):
    """-> (totals int64 [n_groups + 1, 2, 8], loss float64 [n_groups + 1, 2], ratios float32 [n_groups + 1, 2, 6]): the integer
    totals, the fp64 loss sums in table order and gpe_stitch_eval_finalize's ratios; the last row covers every garment"""
    records = np.asarray(records, np.float64)
    totals = np.zeros((n_groups + 1, 2, len(TOTALS)), np.int64)
    loss = np.zeros((n_groups + 1, 2), np.float64)
    for row in range(n_groups + 1):
        for g, r in enumerate(records):
            if not (row == n_groups or (groups is not None and int(groups[g]) == row)) or r[0] != 0.0:
                continue
            for i in ((0, 1) if r[1] != 0.0 else (0,)):
                totals[row, i, :7] += r[3:10].astype(np.int64)
                totals[row, i, 7] += 1
                loss[row, i] = loss[row, i] + r[2]
    ratios = np.zeros((n_groups + 1, 2, len(METRICS)), np.float32)
    for row in range(n_groups + 1):
        for i in range(2):
            pairs, correct, tp, pred, gtp, sel_tp, sel = (int(v) for v in totals[row, i, :7])
            ratios[row, i] = [np.float32(loss[row, i] / np.float64(pairs)) if pairs else np.float32(0), ratio32(correct, pairs),
                              ratio32(tp, pred), ratio32(tp, gtp), ratio32(sel_tp, sel), ratio32(sel_tp, gtp)]
    return totals, loss, ratios


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ---- the chain: prediction -> decoded pattern -> placed edges -> classifier against the pattern's own stitches -------------------------
def chain(preds, data_stats, gt, state_dict, f_shift, f_scale, labels='ground_truth', slot=0):
    """-> (garments as `garment` makes them, per-garment detail [{'logits', 'pairs', 'evaluation', 'n_labels'}]); the class of every
    pair comes from the fp64 logits, so a caller compares counts exactly only where they keep a margin from 0"""
    if labels == 'ground_truth':
        dec = D.restate(preds, data_stats, False, stitches=gt['stitches'], num_stitches=None)[0]
    else:
        dec = D.restate(preds, data_stats, False)[0]
    placed = PL.restate(dec)[0]
    B, P = dec['num_edges'].shape
    L = dec['curved'].shape[2]
    gt_panels = np.asarray(gt['num_panels']).reshape(B)
    out, detail = [], []
    for b in range(B):
        ne = dec['num_edges'][b]
        first, num = int(dec['first_invalid'][b]), int(dec['num_stitches'][b])
        n = first if first >= 0 else num
        pairs = R.enumerate_pairs(ne)
        lg = R.logits64(state_dict, R.pair_rows(placed['edges3d'][b], pairs), f_shift, f_scale) if pairs else np.zeros(0)
        ev = EV.evaluate(pairs, lg, EV.stitches_from_ids(dec['stitches'][b], n, L))
        c = ev['counts']
        out.append(garment([c[k] for k in COUNTS], ev['loss_sum'], c['selected'], num, first, int(dec['num_panels'][b]),
                           int(gt_panels[b]), ne, placed['place_flags'][b], slot))
        detail.append({'logits': lg, 'pairs': pairs, 'evaluation': ev, 'n_labels': n})
    return out, detail
